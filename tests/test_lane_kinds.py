"""CPU: the corpus of tests/lane_kinds.py is what it says -- the oracle alone parses its well-formed
blocks to OK and rejects each malformed one as a parse error (types.rs:315-376, data.rs:43-52)."""
import lane_kinds as K
import oracle as O


def test_oracle_verdicts():
    bins, names = K.corpus()
    assert len(bins) == 16 and names[-5:] == list(K.MALFORMED)
    assert all(len(b) > 10240 + 8 for b in bins[:11]) and all(len(b) > 10240 for b in bins)
    st = [r[0] for r in K.oracle_results()]
    assert st[:11] == [O.BLOCK_OK] * 11, list(zip(names, st))
    assert st[11:] == [O.BLOCK_PARSE_ERROR] * 5, list(zip(names, st))
