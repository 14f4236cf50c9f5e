"""ONE fit per configuration, N = 50 000 fp64, for a kernel trace of the covariance kernels (rocprofv3 --kernel-trace --stats):
  seard      d = 8, SEArd                                   cov_leaf_kernel<double, 8, FAM_SE>         (the bench's kernel: the yardstick)
  seiso1     d = 1, SEIso                                   cov_leaf_kernel<double, 4, FAM_SE>
  periodic1  d = 1, Periodic                                cov_leaf_kernel<double, 4, FAM_PERIODIC>
  maunaloa   d = 1, SE + Periodic * SE + RQ + SE            cov_multi_kernel<double, 4, 5>             (docs/src/mauna_loa.md's tree)
  c3         d = 8, (SEArd + Mat52Iso) + Noise              cov_multi_kernel<double, 8, 2>             (BASELINE configs[2])
Every configuration has its own kernel instantiation, so the trace's per-kernel stats separate them.
usage: periodic_cov.py [config ...] [--n N]   (default: all five, in the order above)"""
import math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gaussianprocesses.jl_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import gpmi355x as g

args = sys.argv[1:]
n = 50000
if "--n" in args:
    i = args.index("--n")
    n = int(args[i + 1])
    del args[i:i + 2]
which = args or ["seard", "seiso1", "periodic1", "maunaloa", "c3"]
for w in which:
    d = 8 if w in ("seard", "c3") else 1
    rng = np.random.default_rng(20240501)
    if d == 1:  # decimal years, as the Mauna Loa data: 46 years, points 0.3 days apart on average
        x = np.sort(rng.uniform(1958.0, 2004.0, size=(1, n)), axis=1)
        y = np.sin(2 * np.pi * x[0]) + 0.01 * (x[0] - 1958.0) ** 2 + 0.1 * rng.standard_normal(n)
    else:
        x = rng.uniform(size=(d, n))
        y = np.sin(2 * np.pi * x).sum(axis=0) / d + 0.1 * rng.standard_normal(n)
    ll = [math.log(0.5) + 0.05 * k for k in range(d)]
    spec = {
        "seard": ("se_ard", ll, 0.0),
        "seiso1": ("se_iso", math.log(2.0), 0.0),
        "periodic1": ("periodic", 0.0, 0.0, 0.0),
        "maunaloa": ("sum", ("sum", ("sum", ("se_iso", 4.0, 4.0), ("prod", ("periodic", 0.0, 1.0, 0.0), ("se_iso", 4.0, 0.0))),
                             ("rq_iso", 0.0, 0.0, -1.0)), ("se_iso", -2.0, -2.0)),
        "c3": ("sum", ("sum", ("se_ard", ll, 0.0), ("mat52_iso", math.log(0.7), math.log(0.5))), ("noise", math.log(0.05))),
    }[w]
    try:
        gp = g.GP(x, y, g.MeanZero(), g.from_spec(spec), math.log(0.1))
        print(w, "n", n, "mll", gp.mll, flush=True)
    except g.PosDefException as e:  # the covariance kernels have run; the trace still has them
        print(w, "n", n, "not positive definite:", e, flush=True)
    del x, y
