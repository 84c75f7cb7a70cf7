"""Writes tests/golden/grad_noise.json: how far the reference's own fp32 autograd sits from the fp64 oracles, per family, fixture and
tensor, and how much of each tensor the whole-tensor gradient gates cannot see.

Reads only the committed fixtures (tests/golden/*.npz, keys ``grad:*``) and the oracles, through tests/grad_cases.py; needs neither
the reference tree nor a GPU.  Two tables, both family -> fixture -> tensor -> number, over the live tensors (those not zero in exact
arithmetic, tests/grad_gate.py::zero_in_exact_arithmetic):

  noise_over_max          max_e |ref32_e - g64_e| / max_e |g64_e|: the floor of tests/grad_gate.py::floor_for is 16 x this
  share_below_1e-3_of_max the share of the tensor's elements with |g64_e| < 1e-3 max|g64|: what max|got - ref| / max|ref| < 5e-4..1e-3
                          leaves unchecked

tests/test_grad_gate_cpu.py recomputes both and requires agreement to 1 %.

    python tests/golden/make_grad_noise.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import grad_cases as GC      # noqa: E402
import grad_gate as GG       # noqa: E402

OUT = os.path.join(HERE, "grad_noise.json")
SMALL = 1e-3


def measure(c):
    """(noise / max|g64|, share of elements below 1e-3 of the largest) per live tensor of one case."""
    nz, sh = {}, {}
    for k in c.live:
        g = c.g64[k]
        m = float(np.abs(g).max())
        nz[k] = GG.noise(c.ref32[k], g) / m
        sh[k] = float(np.mean(np.abs(g) < SMALL * m))
    return nz, sh


def tables():
    out = {"noise_over_max": {}, "share_below_1e-3_of_max": {}}
    for fam, name in GC.all_cases():
        nz, sh = measure(GC.case(fam, name))
        out["noise_over_max"].setdefault(fam, {})[name] = nz
        out["share_below_1e-3_of_max"].setdefault(fam, {})[name] = sh
    return out


if __name__ == "__main__":
    with np.errstate(over="ignore"):
        t = tables()
    with open(OUT, "w") as f:
        json.dump(t, f, indent=1, sort_keys=True)
        f.write("\n")
    for fam, fx in t["noise_over_max"].items():
        allv = [v for d in fx.values() for v in d.values()]
        worst = max(((v, n, k) for n, d in fx.items() for k, v in d.items()))
        share = max(((v, n, k) for n, d in t["share_below_1e-3_of_max"][fam].items() for k, v in d.items()))
        print(f"{fam:9s} noise/max: median {np.median(allv):.2e} worst {worst[0]:.2e} ({worst[1]} {worst[2]});"
              f" worst share below 1e-3 of max {share[0]:.2f} ({share[1]} {share[2]})")
