"""Freeze the reference GMS matcher's answers for the machines that have no reference tree: tests/golden/gms_ref.json.

Per case: the generator (tests/gms_cases.py: kind + arguments), the SHA-256 of the generated input arrays, and the inlier mask the
COMPILED REFERENCE returns (oracle/_ref/libgms_ref.so, `make ref`; bits packed, hex).  Cases: every constructed case of
gms_cases.CONSTRUCTED plus a few of the fuzz.  Needs the compiled reference; refuses inputs on which it leaves its tables.

    python tests/golden/make_golden_gms.py
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import gms_cases as G      # noqa: E402
import gms_ref_lib as R    # noqa: E402

FUZZ_SEEDS = (3, 141, 592, 653, 1589, 1793)


def main():
    if R.load() is None:
        sys.exit("the compiled reference (oracle/_ref/libgms_ref.so) is not available: run `make ref` next to a reference tree")
    named = [(name, kind, args) for name, (kind, args) in G.CONSTRUCTED.items()]
    named += [(f"fuzz_{s}",) + G.fuzz_case(s) for s in FUZZ_SEEDS]
    cases = []
    for name, kind, args in named:
        args = json.loads(json.dumps(args))
        c = G.generate(kind, args)
        mask, flag = R.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        if flag != R.FLAG_NONE:
            sys.exit(f"{name}: the reference left its tables (flag {flag}); not a golden case")
        cases.append(dict(name=name, kind=kind, args=args, n=len(mask), n_inliers=int(mask.sum()), sha256=G.digest(c),
                          mask_hex=np.packbits(mask).tobytes().hex()))
    out = dict(what="inlier masks of the reference's gms_matcher::GetInlierMask(mask, false, false), compiled unchanged (make ref)", cases=cases)
    (HERE / "gms_ref.json").write_text(json.dumps(out, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(cases)} cases -> {HERE / 'gms_ref.json'}")


if __name__ == "__main__":
    main()
