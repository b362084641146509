"""Kernel by kernel comparison of two builds' device assembly and resource usage.

    python tools/isa_diff.py <dir-a> <dir-b> [file.hip ...]

Each directory holds, per source, <file>.s (hipcc --cuda-device-only -S with the product flags of
mysticeti_amd/build.py) and <file>.rpass (the stderr of -Rpass-analysis=kernel-resource-usage).
A kernel's instruction stream is its lines without labels' numbering, comments, directives and
debug lines; 'identical' means the two streams are equal line for line.
"""
import os
import re
import sys

FIELDS = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def key(name: str) -> str:
    # a template kernel's name up to its arguments (parameter types may be renamed between builds)
    return name.split("EvP", 1)[0] + "E" if "EvP" in name else name


def streams(path: str) -> dict:
    s = open(path).read()
    out = {}
    for fn in re.findall(r"^(_Z\S+):", s, re.M):
        if fn.endswith(".const") or ".Lfunc_end" not in s.split(fn + ":", 1)[1]:
            continue
        body = s.split(fn + ":", 1)[1].split(".Lfunc_end", 1)[0]
        lines = []
        for line in body.splitlines():
            line = line.split(";", 1)[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[key(fn)] = lines
    return out


def usage(path: str) -> dict:
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z][^:]*): (\S+))", line)
        if not m:
            continue
        if m.group(1):
            cur = out.setdefault(key(m.group(1)), {})
        elif cur is not None and m.group(2).strip() in FIELDS:
            cur[m.group(2).strip()] = m.group(3)
    return out


def main() -> None:
    a, b = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or sorted(f[:-2] for f in os.listdir(a) if f.endswith(".s"))
    for f in files:
        sa, sb = streams(os.path.join(a, f + ".s")), streams(os.path.join(b, f + ".s"))
        ua, ub = usage(os.path.join(a, f + ".rpass")), usage(os.path.join(b, f + ".rpass"))
        same = [k for k in sa if k in sb and sa[k] == sb[k]]
        print(f"== {f}: {len(sa)} kernels / {len(sb)} kernels, {len(same)} with identical instruction streams")
        for k in sorted(set(sa) ^ set(sb)):
            print(f"  only in {'A' if k in sa else 'B'}: {k}")
        for k in sorted(k for k in sa if k in sb and sa[k] != sb[k]):
            d = {x: (ua.get(k, {}).get(x), ub.get(k, {}).get(x)) for x in FIELDS}
            changed = {x: v for x, v in d.items() if v[0] != v[1]}
            print(f"  DIFF {k}: instructions {len(sa[k])} -> {len(sb[k])}; "
                  f"VGPRs {d['VGPRs'][1]}, LDS {d['LDS Size [bytes/block]'][1]}, scratch {d['ScratchSize [bytes/lane]'][1]}, "
                  f"occupancy {d['Occupancy [waves/SIMD]'][1]}; resource changes: {changed or 'none'}")
        for k in sorted(same):
            if ua.get(k) != ub.get(k):
                print(f"  identical stream, resource report differs {k}: {ua.get(k)} {ub.get(k)}")
        if same:
            print("  identical: " + " ".join(sorted(same)))


if __name__ == "__main__":
    main()
