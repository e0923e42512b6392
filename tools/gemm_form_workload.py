"""The workload behind profiles/gemm_form_kernel_stats*.csv: smoke() plus one Depth Pro default-configuration infer at B = 8 in bf16.
Run it under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) at two commits and compare the "kernel name -> calls"
tables: a change that only moves host code launches the same kernels the same number of times.
usage: gemm_form_workload.py [REPO_ROOT]"""
import os
import sys

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)

import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
from burn_depth_amd import weights as Wt  # noqa: E402
from burn_depth_amd.config import DepthProConfig  # noqa: E402
from burn_depth_amd.depth_pro import DepthPro, Device  # noqa: E402

assert os.path.dirname(os.path.abspath(entry.__file__)) == root
entry.smoke()
cfg = DepthProConfig()
cfg.precision = 0
cfg.max_batch = 8
m = DepthPro.new(Device(0), cfg, seed=0, init_scheme=Wt.INIT_PARITY)
torch.manual_seed(0)
out = m.infer(torch.randn(8, 3, 1536, 1536, device="cuda"))
torch.cuda.synchronize()
assert bool(torch.isfinite(out.depth).all())
m.destroy()
print("workload done", root)
