"""The gap screen alone on a synthetic list B (``sq_gap_screen``, csrc/
estep_f32.hip gap_screen_kernel): device time per launch from HIP events.

The list has the headline's shape by default: 1.14M random rows of a 10M x 256
fp16 array, a ring of 8 shift operands of k = 1024 centroids, candidate sets of
2 / 3 / 4 per row in the given proportions.  The records' gaps sit far above
the threshold, so every row resolves; rows whose base is ring / 2 iterations
old or more get their record rebased, and records and flags are restored
before every launch, so every launch does the same work.  With
``SQ_NATIVE_VARIANT`` naming a variant
library (``python -m sq_learn_amd._build --define SQ_GAP_REDUCE=0 --out ...``)
the same list times that variant; the timing-only variants compute wrong sums,
which this script does not look at."""
import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch

from sq_learn_amd.ops import kmeans as K

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--d", type=int, default=256, help="d_pad: a multiple of 128")
ap.add_argument("--k", type=int, default=1024)
ap.add_argument("--ring", type=int, default=8)
ap.add_argument("--rows", type=int, default=1_140_000, help="length of list B")
ap.add_argument("--wide", type=float, nargs=2, default=[0.35, 0.12],
                help="share of the rows with 3 and with 4 candidates")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--grid", type=int, default=0, help="grid override in blocks (0: the launcher's)")
a = ap.parse_args()

dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
n, d, k, ring, it_now, alpha, delta = a.n, a.d, a.k, a.ring, 9, 1.0, 0.5
Xh = torch.empty((n, d), dtype=torch.float16, device=dev)
for s in range(0, n, 1 << 20):
    e = min(n, s + (1 << 20))
    Xh[s:e] = torch.randn(e - s, d, device=dev, generator=g).to(torch.float16)
xn = torch.full((n,), float(d), dtype=torch.float32, device=dev)
dsh = (torch.randn(ring, k, d, device=dev, generator=g) * 1e-3).to(torch.float16)
dq = torch.zeros((ring, k, 8), dtype=torch.float32, device=dev)
dq[:, :, 2] = 1e-3 * d ** 0.5
dq[:, :, 3] = 1e-7
dq[:, :, 4] = 1.0
rows = torch.randperm(n, device=dev, generator=g)[:a.rows].sort().values
m = rows.numel()
u = torch.rand(m, device=dev, generator=g)
c_r = 2 + (u < a.wide[0] + a.wide[1]).long() + (u < a.wide[1]).long()
jc = torch.randint(0, k, (m, 4), device=dev, generator=g)
jc = torch.where(torch.arange(4, device=dev)[None, :] < c_r[:, None], jc, jc[:, :1])
rec = torch.zeros((n, 8), dtype=torch.float32, device=dev)
r = torch.zeros((m, 8), dtype=torch.float32, device=dev)
r[:, 0], r[:, 1] = 50.0, 1e-3
r[:, 3:6] = 100.0                                     # slot 0 is the argmin, the rest far above
ids = r.view(torch.int32)
ids[:, 6] = (jc[:, 0] | jc[:, 1] << 16 | (c_r - 1) << 30).to(torch.int32)   # wraps to the bit pattern
ids[:, 7] = (jc[:, 2] | jc[:, 3] << 16).to(torch.int32)
rec[rows] = r
mflag = torch.zeros(n, dtype=torch.int32, device=dev)
# bases it_now - (1 .. ring - 1): every ring slot but the current one; rows of
# age >= ring / 2 are rebased (their record is rewritten), the others store nothing
age = torch.randint(1, ring, (m,), device=dev, generator=g)
mflag[rows] = (it_now - age + 2).to(torch.int32)
labels = torch.zeros(n, dtype=torch.int32, device=dev)
labels[rows] = jc[:, 0].to(torch.int32)
rows_b = torch.zeros(n, dtype=torch.int64, device=dev)
rows_b[:m] = rows
count_b = torch.tensor([m], dtype=torch.int32, device=dev)
multi_rows = torch.empty(n, dtype=torch.int64, device=dev)
counts = torch.zeros(3, dtype=torch.int32, device=dev)
rows_mv = torch.empty(n, dtype=torch.int64, device=dev)
rec0, mflag0 = rec.clone(), mflag.clone()
records = K.multi_records(rec=rec, mflag=mflag, it_now=it_now, it_lo=it_now, dsh=dsh, dq=dq,
                          rows_b=rows_b, count_b=count_b, n_done=counts[1:2],
                          rows_moved=rows_mv, count_moved=counts[2:3])


times = []
for i in range(a.warmup + a.iters):
    rec.copy_(rec0)          # rebased rows get their record back: every launch the same work
    mflag.copy_(mflag0)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    counts.zero_()
    t0.record()
    K.gap_screen_native(Xh, xn, labels, multi_rows, counts[0:1], records, alpha, delta,
                        grid_blocks=a.grid)
    t1.record()
    torch.cuda.synchronize()
    if i >= a.warmup:
        times.append(t0.elapsed_time(t1) * 1e3)
fw, done, mv = counts.tolist()
times.sort()
print(f"gap_screen d_pad={d} rows={m} resolved={done} forwarded={fw} moved={mv} "
      f"us mean={sum(times) / len(times):.1f} min={times[0]:.1f} median={times[len(times) // 2]:.1f} "
      f"max={times[-1]:.1f} variant={os.environ.get('SQ_NATIVE_VARIANT', '-')}")
