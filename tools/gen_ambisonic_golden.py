"""Golden vectors for third-order ambisonics (build container only).

`tools/gen_spatial_golden.py`'s construction with the 16 gains of
`spatial.ambisonic(3)` on the reference's own jittered directions: the real
`renderer_cpu.AVRRender` behind a stub network that returns
`signal.float() * Y_k(dir_r)` is channel k of the ambisonic render.  As there,
a case is refused unless the repository's oracle reproduces the reference bit
for bit.  Writes data-only fixtures to `tests/golden/ambisonic/*.npz` (their
own directory: `tests/golden/spatial/*.npz` is one test's glob).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ambisonic_golden.py [case ...]
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_spatial_golden as gsg  # noqa: E402  (puts the repository root on sys.path)

from avr_amd import spatial  # noqa: E402

OUT = os.path.join(gsg.gg.OUT, "ambisonic")


def gain_sh3(w, seed, dirs, inp):
    return spatial.ambisonic(3)(dirs)


CASES = {
    "c1_sh3": (gsg.C1.replace(batch=2), 15, gain_sh3),
}


def main(argv):
    os.makedirs(OUT, exist_ok=True)
    gsg.OUT = OUT  # run_case writes there
    for n in argv or list(CASES):
        gsg.run_case(n, *CASES[n])


if __name__ == "__main__":
    main(sys.argv[1:])
