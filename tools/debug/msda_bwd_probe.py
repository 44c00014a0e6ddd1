"""MSDA backward, time per call.  Default: the TransFusion training shape (24 images x ~10 k padded queries, 8 heads x 4 points,
128 ch on 112 x 200), with the reference points of a third of the queries at (0, 0) like the unseen voxels' and the padded rows'.
Switches (environment, so that the same file also runs against an older tree):
  N, LQ, HOT           maps, queries per map, share of the queries on reference point (0, 0)
  M, D, P              heads, channels per head, points per level
  LEVELS               the levels' maps, e.g. LEVELS=100x134,50x67,25x34,13x17 (default 112x200)
  MODE                 binned | atomic | sorted: sets DF3D_MSDA_BWD for the run (default: leave the variable as it is)
  WINDOWS, CALLS       timed windows and calls per window (default 7 x 10 after 3 warm-up calls); the median window is reported
                       with the fastest and the slowest"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "3d-dual-fusion_amd")]
if os.environ.get("MODE"):
    os.environ["DF3D_MSDA_BWD"] = os.environ["MODE"]
import torch
from dualfusion import ops
dev = torch.device("cuda:0")
N, Lq = int(os.environ.get("N", 24)), int(os.environ.get("LQ", 10000))
M, D, P = int(os.environ.get("M", 8)), int(os.environ.get("D", 16)), int(os.environ.get("P", 4))
maps = [tuple(int(v) for v in m.split("x")) for m in os.environ.get("LEVELS", "112x200").split(",")]
L, S = len(maps), sum(h * w for h, w in maps)
starts = [sum(h * w for h, w in maps[:l]) for l in range(L)]
g = torch.Generator(device="cpu").manual_seed(0)
value = torch.randn(N, S, M, D, generator=g).to(dev)
ref = torch.rand(N, Lq, 1, 1, 1, 2, generator=g)
HOT = float(os.environ.get('HOT', '0.3333'))
if HOT > 0: ref[:, int(Lq * (1 - HOT)):] = 0.0
loc = (ref + torch.randn(N, Lq, M, L, P, 2, generator=g) * 0.01).to(dev).contiguous()
aw = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).to(dev).contiguous()
go = torch.randn(N, Lq, M * D, generator=g).to(dev)
go[:, Lq * 5 // 6:] = 0.0                          # padded rows: no upstream gradient
shp = torch.tensor(maps, dtype=torch.long, device=dev)
ls = torch.tensor(starts, dtype=torch.long, device=dev)
def run():
    return ops.ms_deform_attn_backward(value, shp, ls, loc, aw, go)
plan = ops.msda_backward_plan(N, S, M, D, Lq, L, P, maps, starts) if hasattr(ops, "msda_backward_plan") else "-"
for _ in range(3): out = run()
torch.cuda.synchronize()
WINDOWS, CALLS = int(os.environ.get("WINDOWS", 7)), int(os.environ.get("CALLS", 10))
us = []
for _ in range(WINDOWS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS): out = run()
    b.record(); torch.cuda.synchronize()
    us.append(a.elapsed_time(b) * 1000.0 / CALLS)
us.sort()
print("N=%d Lq=%d M=%d D=%d P=%d levels=%s hot=%s mode=%s plan=%s  %.1f us per call (median of %d windows x %d calls; %.1f .. %.1f);"
      " grad_value checksum %.9e" % (N, Lq, M, D, P, ",".join("%dx%d" % m for m in maps), os.environ.get("HOT", "0.33"),
                                     os.environ.get("DF3D_MSDA_BWD", "default"), plan, us[len(us) // 2], WINDOWS, CALLS, us[0], us[-1],
                                     float(out[0].double().sum())))
