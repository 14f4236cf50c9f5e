"""Wall time of gpmi_grad, gpmi_loo_grad and gpmi_cvfold_grad (folds of 2000) for SEArd d = 8 fp64, and the MFMA products'
share of the gpmi_mfma_peak ceiling from the profile classes (GPMI_PROF_SYRK + GPMI_PROF_PANEL: the CV call minus the gradient
call is the S S' product and its chunked accumulation).  Usage: python tools/cv_time.py [N ...]  (default 20000 50000)"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gaussianprocesses.jl_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gpmi355x as g  # noqa: E402
from bench import synthetic_inputs  # noqa: E402

SYRK, PANEL = 0, 2


def timed(ctx, fn):
    """wall time of one call and the (launches, ms, flops) it added to each class"""
    ctx.profile_enable(True, skip_chain=True)
    ctx.synchronize()
    before = {c: ctx.profile_get(c) for c in (SYRK, PANEL)}
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    dt = time.perf_counter() - t0
    cls = {c: tuple(a - b for a, b in zip(ctx.profile_get(c), before[c])) for c in (SYRK, PANEL)}
    ctx.profile_enable(False)
    return dt, cls


def main(sizes):
    ctx = g.Context.default(0)
    peak = ctx.mfma_peak(64)
    print(f"gpmi_mfma_peak fp64: {peak:.1f} TFLOP/s")
    for n in sizes:
        x, y, _ = synthetic_inputs(n, 8, 16)
        ll = [math.log(0.5) + 0.05 * k for k in range(8)]
        gp = g.GP(x, y, g.MeanZero(), g.SEArd(ll, 0.0), math.log(0.1), ctx=ctx)
        folds = [list(range(k, min(k + 2000, n))) for k in range(0, n, 2000)]
        gp.update_dmll()  # scratch allocated, code loaded
        g.dlogpdθ_LOO(gp, noise=True, domean=False, kern=True)
        g.dlogpdθ_CVfold(gp, folds, noise=True, domean=False, kern=True)
        tg, pg = timed(ctx, gp.update_dmll)
        tl, pl = timed(ctx, lambda: g.dlogpdθ_LOO(gp, noise=True, domean=False, kern=True))
        tf, pf = timed(ctx, lambda: g.dlogpdθ_CVfold(gp, folds, noise=True, domean=False, kern=True))
        print(f"N={n}: gpmi_grad {1e3 * tg:.1f} ms, gpmi_loo_grad {1e3 * tl:.1f} ms ({tl / tg:.2f}x), "
              f"gpmi_cvfold_grad ({len(folds)} folds) {1e3 * tf:.1f} ms ({tf / tl:.2f}x LOO)")
        for name, p in (("loo", pl), ("folds", pf)):
            ms = sum(p[c][1] - pg[c][1] for c in (SYRK, PANEL))
            work = sum(p[c][2] - pg[c][2] for c in (SYRK, PANEL))
            if ms > 0:
                print(f"  {name}: S S' products {ms:.1f} ms, {work / ms / 1e9:.1f} TFLOP/s = {work / ms / 1e9 / peak:.2f} of peak")
        del gp


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [20000, 50000])
