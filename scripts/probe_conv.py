"""Timing of the convolution objective's kernels: python scripts/probe_conv.py [K] [nt] [out file].

Times conv_eval_tensors for K restarts (HIP events on the library's stream after a warm-up), J-only (k_conv_mm
forward + k_conv_J) and J + df (+ k_conv_mm adjoint) separately, against two yardsticks on the same data:
  * the same computation as dense torch.float64 matmuls with the explicit K and M on the same GPU (twice the flops:
    the zero triangle is multiplied too, and K streams from HBM);
  * numpy on 16 CPU threads (threadpoolctl when present, else whatever the BLAS was started with).
Prints the three timings, the TFLOP/s counted on the triangular flops (nt·(nt+1) per product per restart) and the
fraction of the FP64 MFMA peak (78.6 TFLOP/s, AMD's figure), and checks restarts 0 and K-1 against numpy.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd"), ROOT]
os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mioc import native  # noqa: E402
from mioc.conv import ConvProblem  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
out = sys.argv[3] if len(sys.argv) > 3 else None
REP = 20
PEAK = 78.6

cp = ConvProblem(nt=nt)
ctx = native.Context(0)
cp.setup(ctx)
g = torch.Generator().manual_seed(5)
# piecewise constant over 16 steps, levels -2..2
x = torch.randint(-2, 3, (K, (nt + 15) // 16, 1), generator=g).double().repeat_interleave(16, dim=1)
x = x[:, :nt].contiguous().cuda()
J = torch.empty(K, dtype=torch.float64, device="cuda")
df = torch.empty_like(x)
st = torch.cuda.ExternalStream(ctx.stream())


def time_dev(fn):
    for _ in range(3):
        fn()
    ctx.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(st)
    for _ in range(REP):
        fn()
    ev[1].record(st)
    ctx.synchronize()
    return ev[0].elapsed_time(ev[1]) / REP


ms_J = time_dev(lambda: ctx.conv_eval_tensors(x, J, None))
ms_Jdf = time_dev(lambda: ctx.conv_eval_tensors(x, J, df))

# yardstick 1: dense torch.float64 on the same GPU (explicit K and M)
Kn, Mn = cp.dense()
Kd, Md, fd = (torch.tensor(a, dtype=torch.float64, device="cuda") for a in (Kn, Mn, cp.fvec))
X2 = x[:, :, 0]


def torch_J():
    v = X2 @ Kd.T - fd
    return 0.5 * ((v @ Md) * v).sum(dim=1), v


def torch_Jdf():
    Jt, v = torch_J()
    return Jt, (v @ Md) @ Kd


def time_torch(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(REP):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / REP


ms_tJ = time_torch(lambda: torch_J()[0])
ms_tJdf = time_torch(torch_Jdf)
Jt, dft = torch_Jdf()

# yardstick 2: numpy on 16 CPU threads
try:
    from threadpoolctl import threadpool_limits
    limit = threadpool_limits(limits=16)
except ImportError:
    limit = None
Xn = X2.cpu().numpy()


def numpy_Jdf():
    v = Xn @ Kn.T - cp.fvec
    w = v @ Mn
    return 0.5 * np.sum(w * v, axis=1), w @ Kn


numpy_Jdf()
t0 = time.perf_counter()
Jn, dfn = numpy_Jdf()
ms_np = (time.perf_counter() - t0) * 1e3

ok = True
Jh, dfh = J.cpu().numpy(), df.cpu().numpy()[:, :, 0]
for k in (0, K - 1):
    ok &= abs(Jh[k] - Jn[k]) <= 1e-9 * abs(Jn[k])
    ok &= np.max(np.abs(dfh[k] - dfn[k])) <= 1e-9 * np.max(np.abs(dfn[k]))
ok &= bool(torch.allclose(Jt, J, rtol=1e-9, atol=0.0))
tri = 1.0 * nt * (nt + 1) * K  # flops of one triangular product (a multiply-add = 2, half the entries)
tf_J, tf_Jdf = tri / (ms_J / 1e3) / 1e12, 2 * tri / (ms_Jdf / 1e3) / 1e12
lines = [
    f"probe_conv: K={K} nt={nt} (HIP events, {REP} launches after 3 warm-up; parity={'ok' if ok else 'FAIL'})",
    f"  libmioc  J only  {ms_J:8.3f} ms  {tf_J:6.2f} TFLOP/s on the triangular flops = {tf_J / PEAK:.3f} of FP64 MFMA peak",
    f"  libmioc  J + df  {ms_Jdf:8.3f} ms  {tf_Jdf:6.2f} TFLOP/s on the triangular flops = {tf_Jdf / PEAK:.3f} of FP64 MFMA peak",
    f"  torch dense f64, same GPU   J only {ms_tJ:8.3f} ms   J + df {ms_tJdf:8.3f} ms   "
    f"(torch / libmioc = {ms_tJ / ms_J:.2f} / {ms_tJdf / ms_Jdf:.2f})",
    f"  numpy dense f64, 16 CPU threads{'' if limit is not None else ' (OMP_NUM_THREADS)'}   J + df {ms_np:8.1f} ms   "
    f"(numpy / libmioc = {ms_np / ms_Jdf:.0f})",
]
print("\n".join(lines), flush=True)
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
ctx.close()
