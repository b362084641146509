// tools/propose_probe.py's helper: the include choice of Core::try_new_block (core.rs:254-271) as the
// reference makes it on the core thread -- a HashSet of BlockReference filled from the own last
// block's includes and from every taken block's includes, then one lookup per taken include -- restated
// with std::unordered_set on one host core. A reference is six words (authority, round, digest).
#include <stdint.h>

#include <chrono>
#include <unordered_set>

namespace {
struct Ref {
  uint64_t w[6];
  bool operator==(const Ref& o) const {
    for (int i = 0; i < 6; i++)
      if (w[i] != o.w[i]) return false;
    return true;
  }
};
struct RefHash {
  size_t operator()(const Ref& r) const {
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the words
    for (int i = 0; i < 6; i++) h = (h ^ r.w[i]) * 0x100000001b3ull;
    return (size_t)h;
  }
};
}  // namespace

// own: n_own references; taken: n_taken references; inc / inc_off: the includes of taken block i are
// inc[6 * inc_off[i]] .. inc[6 * inc_off[i + 1]] (an empty span: get_block gave None). out: the kept
// references, in order (n_taken x 6 words of room). Returns the kept count; *ns = the time it took.
extern "C" uint64_t propose_host_choice(const uint64_t* own, uint64_t n_own, const uint64_t* taken, uint64_t n_taken,
                                        const uint64_t* inc, const uint64_t* inc_off, uint64_t* out, uint64_t* ns) {
  const auto t0 = std::chrono::steady_clock::now();
  std::unordered_set<Ref, RefHash> in_block;
  const Ref* o = reinterpret_cast<const Ref*>(own);
  in_block.insert(o, o + n_own);
  const Ref* all = reinterpret_cast<const Ref*>(inc);
  for (uint64_t i = 0; i < n_taken; i++) in_block.insert(all + inc_off[i], all + inc_off[i + 1]);
  const Ref* t = reinterpret_cast<const Ref*>(taken);
  Ref* dst = reinterpret_cast<Ref*>(out);
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n_taken; i++)
    if (!in_block.count(t[i])) dst[kept++] = t[i];
  *ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  return kept;
}
