"""Freeze the reference GMS matcher's answers WITH scale / rotation for the machines that have no reference tree:
tests/golden/gms_modes_ref.json.

Per case of tests/gms_mode_cases.py: the generator (kind + arguments), the SHA-256 of the generated input arrays and, per flag pair
(with_scale, with_rotation) in ((0, 1), (1, 0), (1, 1)), the inlier mask the COMPILED REFERENCE returns (oracle/_ref/libgms_ref_modes.so,
`make ref_modes`; bits packed, hex), its count and the size of its mask vector (0: no hypothesis kept a match and the reference left
the vector untouched).  Needs the compiled reference; refuses a case on which it leaves its tables.

    python tests/golden/make_golden_gms_modes.py
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import gms_cases as G            # noqa: E402
import gms_mode_cases as MC      # noqa: E402
import gms_modes_ref_lib as R    # noqa: E402


def main():
    if R.load() is None:
        sys.exit("the compiled reference (oracle/_ref/libgms_ref_modes.so) is not available: run `make ref_modes` next to a reference tree")
    cases = []
    for name, (kind, args) in MC.CASES.items():
        args = json.loads(json.dumps(args))
        c = MC.generate(kind, args)
        answers = []
        for ws, wr in MC.FLAG_PAIRS:
            mask, cnt, size, flag = R.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], ws, wr)
            if flag != R.FLAG_NONE:
                sys.exit(f"{name} {(ws, wr)}: the reference left its tables (flag {flag}); not a golden case")
            answers.append(dict(with_scale=ws, with_rotation=wr, n_inliers=cnt, mask_size=size, mask_hex=np.packbits(mask).tobytes().hex()))
        cases.append(dict(name=name, kind=kind, args=args, n=len(c["q"]), sha256=G.digest(c), answers=answers))
    out = dict(what="inlier masks of the reference's gms_matcher::GetInlierMask(mask, with_scale, with_rotation), compiled unchanged (make ref_modes)",
               cases=cases)
    (HERE / "gms_modes_ref.json").write_text(json.dumps(out, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(cases)} cases -> {HERE / 'gms_modes_ref.json'}")


if __name__ == "__main__":
    main()
