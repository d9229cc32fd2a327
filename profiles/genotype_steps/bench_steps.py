"""bench.py's --genotype workload (its own block, priors, warm-up and step loop) of the checkout argv[1] (argv[2]: single | trio), keeping every step: device ms (HIP events),
wall ms, host_prepare_ms; the likelihoods of the last step go to argv[3].npy."""
import json, os, sys, time
tree = os.path.abspath(sys.argv[1]); workload = sys.argv[2]; out = sys.argv[3]
sys.path.insert(0, tree)
os.chdir(tree)
import numpy as np
sys.argv = ["bench.py", "--gpus", "1", "--steps", "9", "--warmup", "2", "--workload", "genotype_trio" if workload == "trio" else "genotype"]
import bench
from whatshap_amd import _native
assert os.path.abspath(bench.__file__).startswith(tree) and os.path.abspath(_native.__file__).startswith(tree)
args = bench.parse_args()
for key, value in bench.WORKLOADS[args.workload].items():   # (as bench.main does)
    setattr(args, key, value)
assert args.genotype
if args.trio and args.coverage == 20:
    args.coverage = 15
v = args.variants or (20000 if args.trio else 50000)
problem = bench.with_uniform_priors(bench.build_block(args, 4 if args.trio else 2, v))
n = int(problem.positions.size)
for _ in range(args.warmup):
    _native.genotype_likelihoods(problem, n)
wall, dev, prep = [], [], []
for _ in range(args.steps):
    t0 = time.perf_counter()
    gl, stats = _native.genotype_likelihoods(problem, n)
    wall.append((time.perf_counter() - t0) * 1e3); dev.append(stats["total_ms"]); prep.append(stats["host_prepare_ms"])
np.save(out, gl)
print("BENCH", json.dumps({"tree": tree, "workload": workload, "n": n, "dev_ms": dev, "wall_ms": wall, "prep_ms": prep,
                           "dev_median": float(np.median(dev)), "wall_median": float(np.median(wall)), "prep_median": float(np.median(prep)),
                           "launches": stats["launches"], "slot_runs": stats["slot_runs"]}), flush=True)
