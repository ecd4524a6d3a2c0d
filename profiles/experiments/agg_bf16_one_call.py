"""The d = 128 forward SpMM of the default model on the symmetric Reddit stand-in, fp32 and bf16, a few calls each --
the target of the rocprofv3 --pmc passes behind DESIGN.md's bf16 counter table (one counter group per run).
Usage: python profiles/experiments/agg_bf16_one_call.py [calls]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
import torch  # noqa: E402

(ip, ix, dv), _, _ = pkg.datasets.synth_reddit_like(1.0, seed=1, symmetric=True)
n = ip.shape[0] - 1
A = pkg.csr_matrix(ip, ix, dv, n)
A.normalize(True)
A = A.transpose()                                   # the forward operand, as gcn() builds it
ctx = pkg.context(0)
plan = pkg.ops.spmm_plan_for(ctx, A, 128, 128)
B = pkg.dn_matrix(n, 128, torch.randn(n * 128, device="cuda"))
B16 = torch.empty((n, 128), dtype=torch.bfloat16, device="cuda")
C = pkg.dn_matrix(n, 128)
for _ in range(calls):
    pkg.matmul(ctx, A, B, C, plan, 1.0, 0.0)
pkg.ops.convert_bf16(ctx, B, B16)
for _ in range(calls):
    pkg.ops.spmm_bf16(ctx, A, B16, C, plan, 1.0, 0.0)
ctx.sync()
print("done", calls, plan.describe().split(" | ")[0])
