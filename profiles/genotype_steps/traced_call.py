"""One small genotyping call with the checkout given as argv[1]: case a / b / c / d of bench.md (argv[2]), likelihoods to argv[3] (.npy), stats on
stdout.  Case b takes its WHAMD_GENO_WINDOW_BYTES from GENO_B_BYTES.  Run under `rocprofv3 --hip-trace --kernel-trace --output-format csv`."""
import json, os, sys
tree = os.path.abspath(sys.argv[1])
case, out = sys.argv[2], sys.argv[3]
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
import numpy as np
from genotype_cases import random_case
from whatshap_amd import _native
assert os.path.abspath(_native.__file__).startswith(tree), _native.__file__
p = random_case(10, mode="trio", n_variants=40, n_reads=120, max_len=7, max_coverage=9)
window = {"a": 0, "b": 0, "c": 64, "d": 3}[case]
if case == "b":
    os.environ["WHAMD_GENO_WINDOW_BYTES"] = os.environ["GENO_B_BYTES"]
gl, stats = _native.genotype_likelihoods(p, 40, window=window)
np.save(out, gl)
print("STATS", case, json.dumps(stats))
