"""One process for the masked product under a STATIC environment switch of grb_mxm (read once per process, so a test
cannot move it in-process): tests/test_gpu_mxm_masked_routes.py starts this file with the switch set.

    GRB_TC_BITMAP_MIN=0  python tests/tools/mxm_masked_child.py compact
        comb, int32, both sides one-valued, PlusMultiplies and PlusMinus: the compact key-only path keeps the pivots
        beyond 2048 entries -- 64 KiB and 128 KiB tables, the pivot in segments
    GRB_MXM_PIVOT=0      python tests/tools/mxm_masked_child.py entry
        comb, both types, valued and one-valued: the entry-driven kernel alone, the whole wave on every long entry

Both the pattern and its mirror, against the reference of tests/mxm_masked_cases.py, bit for bit.  The route model
(which reads the same variables) must confirm that the switch leads where this run is meant to go.  Exit status 0:
everything equal; 1: a mismatch (printed); 2: the environment is not the one the mode needs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root

import mxm_masked_cases as mc                                  # noqa: E402


def main(mode):
    comb = mc.comb()
    if mode == "compact":
        if mc.bitmap_min() != 0 or not mc.pivot_on():
            return 2
        runs = [(np.int32, "iso_ab", sr) for sr in ("PlusMultiplies", "PlusMinus")]
        for case in (comb, comb.mirrored()):
            f = mc.routes(case, np.int32, "iso_ab", "PlusMultiplies")
            for p in (mc.PASS1, mc.PASS2):
                assert f["passes"][p]["compact"] and mc.owned(f, p, "bitmap") == 0
                assert all(mc.owned(f, p, k) > 100 for k in ("table64", "table128", "segments")), f["count"]
    elif mode == "entry":
        if mc.pivot_on():
            return 2
        runs = [(dt, layout, sr) for dt in mc.DTYPES for layout in ("valued", "iso_ab")
                for sr in ("PlusMultiplies", "PlusMinus", "MinimumPlus")]
        f = mc.routes(comb, np.float32, "valued", "PlusMinus")
        assert not f["passes"] and mc.owned(f, mc.ENTRY_ALONE, "heavy") > 3000 and mc.owned(f, mc.ENTRY_ALONE, "lane") > 1000
    else:
        return 2
    import graphblast_amd as g
    status = 0
    for case in (comb, comb.mirrored()):
        for dtype, layout, sr in runs:
            av, bv = mc.operands(case, sr, dtype, layout)
            got = mc.product(g, case, dtype, sr, av, bv, mc.build_mask(g, case, dtype))
            bad = mc.mismatches(case, dtype, layout, sr, got, mc.want(case, sr, dtype, av, bv))
            if bad:
                print(bad)
                status = 1
    print("mxm_masked_child %s: %s" % (mode, "ok" if status == 0 else "MISMATCH"))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
