"""The field-response builder (ldsim_response_build, csrc/kernels_respbuild.hip) on module0's table, (45, 45, 1950), at n_sub 4 and
16: HIP-event time of response_build_kernel as the median of 5 builds after 2 warm-ups (min .. max), the rate in evaluations of
the weighting potential per second, and beside it the wall time of the numpy twin (f64) for the same table on the same machine.
Then the worst |kernel - long-double twin| of the test suite's small cases with the bound the tests hold them to
(tests/test_gpu_response_builder.py: four times the f64 twin's own difference).
python tools/response_build_timing.py [--repeats R] [--out FILE]   (default: profiles/response_build_timing.log)"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "larnd-sim_amd"), REPO):
    sys.path.insert(0, p)

CASES = {"(7, 5, 300) n_sub 3": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=3),
         "(7, 5, 300) n_sub 1": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=1),
         "(7, 5, 300) n_sub 3, pad 0.8 pitch": dict(shape=(7, 5, 300), arrival_tick=280, n_sub=3, pad_frac=0.8),
         "(3, 2, 3800) n_sub 3, 0.05 us": dict(shape=(3, 2, 3800), n_sub=3, sampling=0.05),
         "(7, 7, 1950) n_sub 2": dict(shape=(7, 7, 1950), n_sub=2)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "response_build_timing.log"))
    a = ap.parse_args(argv)
    import numpy as np
    from larndsim_amd import consts, lib, response_builder as RB
    consts.load_snapshot("module0")
    ctx = lib.context()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for n_sub in (4, 16):
        p = RB.params(n_sub=n_sub)
        ms = []
        for k in range(2 + a.repeats):
            table = RB.build(p, ctx)
            if k >= 2:
                ms.append(RB.build_ms(ctx))
        med = float(np.median(ms))
        evals = p["n_i"] * p["n_j"] * (p["n_k"] + 1) * n_sub * n_sub
        t0 = time.perf_counter()
        twin = RB.twin(p)
        wall = time.perf_counter() - t0
        say(f"(45, 45, 1950) n_sub {n_sub}: response_build_kernel {med:.2f} ms ({min(ms):.2f} .. {max(ms):.2f}), "
            f"{evals / med / 1e6:.1f} G potentials/s; numpy twin {wall:.2f} s on the host ({wall * 1e3 / med:.0f} x); "
            f"max |kernel - f64 twin| {np.abs(table - twin).max():.3e}, peak entry {twin.max():.4f}")
    for name, kw in CASES.items():
        kw = dict(kw)
        p = RB.params(pad_size=kw.pop("pad_frac", 1.0) * consts.detector.PIXEL_PITCH, **kw)
        ld = RB.twin(p, np.longdouble)
        say(f"{name}: worst |kernel - long-double twin| {float(np.abs(RB.build(p, ctx) - ld).max()):.3e}, bound "
            f"{4 * float(np.abs(RB.twin(p) - ld).max()):.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
