"""Ignatius, real weights: the last 128 -> 128 layer launched N times on its real input with the L2 / MALL thrashed in between; the quads that differ from the
majority output, and where they sit in their workgroup's tile sequence.  python tools/det_ws_real.py [repeats]"""
import sys, os, numpy as np, torch
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from dgnn_amd import ops
from dgnn_amd.graph import GraphPlan
from test_gpu_parity import hip_static
from helpers import gold
dev = "cuda:0"
g = gold("static_f4_ignatius_full.npz")
n = g["x"].shape[0]
fg = np.random.default_rng(int(g["fgeom_seed"])).standard_normal((4 * n, 4)).astype(np.float32)
ea = torch.from_numpy(np.concatenate([fg, g["edge_attr16"]], axis=1)).to(dev)
pairs = np.stack([np.repeat(np.arange(n, dtype=np.int64), 4), g["adj_dst"].astype(np.int64)], 1)
ei = torch.from_numpy(pairs).to(dev).t().contiguous()
x0 = torch.from_numpy(g["x"]).to(dev)[:, 1:].contiguous()
net = hip_static()
plan = GraphPlan(ei, n, n)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
acts = [x0]
for i in range(4):
    acts.append(net._eval_layers(acts[-1], n, ea, [plan] * 4, True, only=i).clone())
ntiles = (n + 31) // 32
per = (ntiles + 7) // 8
junk = torch.empty(1 << 28, device=dev)        # 1 GiB
print("n", n, "tiles", ntiles, "per XCD", per)
for i in (3, 2):
    outs = []
    for r in range(reps):
        junk.add_(1.0)                         # evicts L2 and MALL
        outs.append(net._eval_layers(acts[i], n, ea, [plan] * 4, True, only=i).clone())
    ref = torch.stack(outs[:5]).median(0).values
    ev = 0
    for r, o in enumerate(outs):
        k = (o != ref).any(1).nonzero().flatten().tolist()
        if k:
            ev += 1
            tiles = sorted(set(c // 32 for c in k))
            for t in tiles[:4]:
                rows = [c % 32 for c in k if c // 32 == t]
                xcd = t // per; rel = t - xcd * per; it = rel // 32; slot = rel % 32
                t_hi = min(ntiles, (xcd + 1) * per); my_n = (t_hi - xcd * per - slot + 31) // 32
                c = t * 32 + rows[0]
                ch = (o[c] != ref[c]).nonzero().flatten().tolist()
                print("  layer %d rep %d tile %d rows %s: xcd %d wg %d it %d of %d; row %d: %d channels %d..%d" % (i, r, t, rows, xcd, slot, it, my_n, rows[0], len(ch), ch[0], ch[-1]))
    print("layer %d: %d of %d launches differ" % (i, ev, reps))
