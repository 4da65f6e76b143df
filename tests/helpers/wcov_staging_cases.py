"""The case list of tests/test_gpu_wcov_staging.py: the pair-list scatter with 64-column chunks (k_wcov_mfma_partial<64, SQ, false, false, NT>), whose staging
is straight-line below the last row tile and guarded in it.  Inputs, references and bounds are those of tests/helpers/mfma_cases.py (imported, the same
file format and harness); tests/test_wcov_staging_cpu.py shows on the CPU that the list reaches what it claims and that a plain float64 evaluation meets
every bound.

Rows: cs = 96 (six full tiles, no ones row), 97 (the last tile holds one data row and the ones row), 100 / 101 (the headline shape and its neighbour),
111 (the ones row is the last row of the last tile), 112 (seven full tiles, no ones row), 20 and 80 (two and five tiles).
Columns: m = 1, 63, 64, 65, 130, 257 in 1, 2 and 6 splits of whole 64-column chunks: a split that is empty, one that ends inside a chunk and one that
ends on a chunk boundary all occur."""
from tests.helpers import mfma_cases as M

CS = (96, 97, 100, 101, 111, 112, 20, 80)
MS = (1, 63, 64, 65, 130, 257)
SPLITS = (1, 2, 6)
SOURCES = ("plain", "w", "cost")
GATHER_K = 600                                            # gathered cases: m of 600 columns (at most half of the columns may appear)


def _contiguous(cs, m, ksplit, source):
    """m contiguous columns (K = m).  A lone column cannot carry the +inf cost the cost variant plants, and K - 1 = 0 is no denominator"""
    if m == 1 and source == "cost":
        source = "w"
    kw = dict(den=1.0) if (m == 1 and source == "plain") else {}
    return dict(cs=cs, K=m, ksplit=ksplit, variant=source, **kw)


def specs():
    """-> list of keyword dicts for mfma_cases.wcov_case"""
    out = []
    # the headline row count against every column count and split count, the weight source rotating so that every m and every split count meets all three
    out += [_contiguous(100, m, ks, SOURCES[(i + j) % 3]) for i, m in enumerate(MS) for j, ks in enumerate(SPLITS)]
    # every other row count: three column counts, three split counts, every weight source
    for i, cs in enumerate(c for c in CS if c != 100):
        ms = [MS[(2 * i + j) % 6] for j in range(3)]
        src = SOURCES if ms[2] != 1 else SOURCES[::-1]                    # (the lone column does not take the costs)
        out += [_contiguous(cs, ms[j], SPLITS[(i + j) % 3], src[j]) for j in range(3)]
    # the ones row off where the shape has room for it (external mean), contiguous columns
    out += [dict(cs=cs, K=m, ksplit=ks, variant=v, want_mu=False) for cs, m, ks, v in ((97, 65, 2, "w"), (100, 130, 6, "plain"), (111, 257, 1, "w"), (20, 63, 2, "plain"))]
    # gathered columns: external mean (as :cemppi takes them), weighted with their sum given, and with the ones row on
    out += [dict(cs=cs, K=GATHER_K, ksplit=ks, variant=v, m=m) for cs, m, ks, v in ((100, 65, 2, "idx"), (97, 130, 6, "idx_w"), (112, 257, 2, "idx"), (80, 63, 1, "idx_w"),
                                                                                  (101, 1, 2, "idx"))]
    out += [dict(cs=cs, K=GATHER_K, ksplit=ks, variant=v, m=m, want_mu=True) for cs, m, ks, v in ((100, 257, 6, "idx_w"), (111, 64, 1, "idx"), (20, 130, 2, "idx"))]
    # the fourth-moment variant at the headline row count
    out += [dict(cs=100, K=GATHER_K, ksplit=ks, variant=v, m=m) for v, m, ks in (("ss", 65, 2), ("lw", 130, 6), ("ss", 257, 1))]
    return out


def case_id(s):
    return "cs%d-m%d-k%d-%s%s" % (s["cs"], s.get("m", s["K"]), s["ksplit"], s["variant"], {None: "", True: "-mean", False: "-nomean"}[s.get("want_mu")])


def build(spec):
    return M.wcov_case(**spec)


def chunk_ends(c):
    """how the splits of a case end -> set of 'empty', 'mid' (inside a 64-column chunk), 'boundary'"""
    per = M.wcov_per(c["cs"], c["m"], c["ksplit"])
    out = set()
    for s in range(c["ksplit"]):
        kbeg, kend = s * per, min(c["m"], s * per + per)
        out.add("empty" if kbeg >= kend else "mid" if (kend - kbeg) % 64 else "boundary")
    return out


def poisoned(c, value=1e300):
    """a gathered case with `value` in every column the range idx[:, :m] does not name, and with idx[:, m:] (the entries after the range) pointing at such
    columns; weights given: `value` there too.  Nothing the scatter may read changes."""
    import numpy as np
    assert c["idx"] is not None and c["m"] < c["K"]
    X, idx = c["X"].copy(), c["idx"].copy()
    w = None if c["w"] is None else c["w"].copy()
    for b in range(c["B"]):
        unused = np.setdiff1d(np.arange(c["K"]), idx[b, :c["m"]])
        assert unused.size
        X[b][:, unused] = value
        if w is not None:
            w[b][unused] = value
        idx[b, c["m"]:] = unused[np.arange(c["K"] - c["m"]) % unused.size]
    op, B, ipar, dpar, arrays = M.unpack_case(c["data"])
    arrays[1], arrays[4] = (M.F64, X), (M.I32, idx)
    if w is not None:
        arrays[2] = (M.F64, w)
    return dict(c, X=X, idx=idx, w=w, data=M.pack_case(op, B, ipar, dpar, [(t, a if a.size else None) for t, a in arrays]))
