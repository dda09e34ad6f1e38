"""Every backward entry of the three decoder families behind every forward pass it takes, at the tiny golden dims (3 images, 4 steps,
K = 2, Philox seeds): the loss outputs and every gradient of each (family, stored pass, entry) written as DIR/<family>.<pass>.<entry>.<name>.npy.
Two builds of the library that launch the same kernels in the same order write the same bits: run it under each and compare the
directories file by file with np.array_equal (--compare OTHER does that and prints one JSON line).  The eager handles only; the
graph twins are pinned against them by tests/test_gpu_backward_entries.py.
usage: dump_backward_heads.py DIR [--compare OTHER]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import butd as ob  # noqa: E402
from simpleimagecaptionzoo_amd.aoa import AoaHandle  # noqa: E402
from simpleimagecaptionzoo_amd.butd import ButdHandle  # noqa: E402
from simpleimagecaptionzoo_amd.distill import xe_backward_distill, xe_backward_dlogits  # noqa: E402
from simpleimagecaptionzoo_amd.grouped import xe_forward_n  # noqa: E402
from simpleimagecaptionzoo_amd.multisample import sample_n  # noqa: E402
from simpleimagecaptionzoo_amd.nic import NicHandle  # noqa: E402
from simpleimagecaptionzoo_amd.scst_objective import make_objective, sample_backward_objective  # noqa: E402
from simpleimagecaptionzoo_amd.swor import SworBatch, xe_backward_swor  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
OUT = sys.argv[1]
if "--compare" in sys.argv:
    other = sys.argv[sys.argv.index("--compare") + 1]
    names = sorted(os.listdir(OUT))
    differ = [n for n in names if not (os.path.exists(os.path.join(other, n)) and np.array_equal(np.load(os.path.join(OUT, n)), np.load(os.path.join(other, n))))]
    missing = sorted(set(os.listdir(other)) - set(names))
    print(json.dumps({"files": len(names), "equal": len(names) - len(differ), "differ": differ, "only_in_other": missing}))
    sys.exit(1 if differ or missing or not names else 0)
if not torch.cuda.is_available():
    sys.exit("dump_backward_heads.py runs on the GPU: no device found")
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
B, T, K, L = 3, 4, 2, 5
LENGTHS, LENGTHS_N = [4, 3, 2], [2, 4, 3, 3, 1, 4]
ROLLOUT_ENTRIES, XE_ENTRIES = ("sample_backward", "sample_backward_objective", "sample_backward_dlogp"), ("xe_backward", "xe_backward_distill", "xe_backward_swor", "xe_backward_dlogits")


def randn(shape, seed, dtype=torch.float32):
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(DEV)


def sd_of(g):
    return {k[3:]: torch.tensor(np.asarray(v), dtype=torch.float32, device=DEV) for k, v in g.items() if k.startswith("sd.")}


def make(family):
    g = dict(np.load(os.path.join(GOLDEN, {"butd": "butd_dec_tiny", "aoa": "aoa_tiny", "nic": "nic_dec_tiny"}[family] + ".npz")))
    dims = [int(x) for x in g["dims"]][1:]
    if family == "butd":
        R, D, H, E, A, V = dims
        h = ButdHandle(R, D, H, E, A, V, 8, 20, DEV)
        h.bind(ob.strip_prefix(sd_of(g)))
        feats = torch.relu(randn((B, R, D), 11))
    elif family == "aoa":
        R, D, Hd, E, V, NH = dims
        h = AoaHandle(R, D, Hd, E, V, NH, 8, 20, DEV)
        h.bind(sd_of(g))
        feats = torch.relu(randn((B, R, D), 14))
    else:
        H, E, V = dims
        h = NicHandle(E, H, V, 8, 20, DEV)
        h.bind(sd_of(g))
        feats = randn((B, E), 12)
    return h, feats, V


def captions(lengths, V, seed):
    rs = np.random.RandomState(seed)
    caps = torch.zeros(len(lengths), L, dtype=torch.int64)
    for b, n in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:n] = torch.from_numpy(rs.randint(4, V, size=n - 1))
        caps[b, n] = 2
    return caps.to(DEV)


def store(h, feats, V, what):
    rng = h._make_rng(4242)
    if what == "sample":
        h.sample(feats, T, rng)
    elif what == "sample_n":
        sample_n(h, feats, K, T, rng)
    elif what == "rollouts":
        h.rollouts(feats, T, rng)
    elif what == "xe":
        h.xe_forward(feats, captions(LENGTHS, V, 15), LENGTHS, rng, train=True)
    else:
        xe_forward_n(h, feats, captions(LENGTHS_N, V, 16), LENGTHS_N, K, rng, train=True)
    return B * K if what in ("sample_n", "xe_n") else B


def backward(h, entry, rows, n_tok, V, grads):
    nic = h.family == "nic"
    kw = {"want_dfeats": True} if nic else {}
    if entry == "sample_backward":
        out = h.sample_backward(randn((rows, 1), 17).repeat(1, T).contiguous(), grads, **kw)
        return dict(zip(("loss", "mask_sum", "dfeats"), out))
    if entry == "sample_backward_objective":
        out = sample_backward_objective(h, make_objective("reinforce", 1, entropy_weight=0.05, reward=randn((rows, T), 18)), grads, want_entropy=True, **kw)
        return dict(zip(("loss3", "mask_sum", "entropy", "dfeats"), out))
    if entry == "sample_backward_dlogp":
        h.sample_backward_dlogp(randn((rows, T), 19), grads)
        return {}
    if entry == "xe_backward":
        out = h.xe_backward(grads, 0.1, **kw)
        return dict(zip(("loss", "dfeats"), out if nic else (out,)))
    if entry == "xe_backward_distill":
        out = xe_backward_distill(h, grads, [randn((n_tok, V), 20)], alpha=0.5, temperature=2.0, **kw)
        return dict(zip(("loss", "hard", "kd", "dfeats"), out))
    if entry == "xe_backward_swor":
        n = rows + 1                        # one image of `rows` samples and its threshold slot
        rs = np.random.RandomState(16)
        phi = torch.from_numpy((-rs.rand(n) * 15.0 - 0.1).astype(np.float32))
        G = torch.from_numpy(np.sort(rs.rand(n) * 10.0 - 12.0)[::-1].copy())
        batch = SworBatch(None, LENGTHS, torch.arange(rows, dtype=torch.int32), torch.arange(rows, dtype=torch.int64).view(1, rows))
        out = xe_backward_swor(h, grads, phi, G, torch.from_numpy(rs.rand(n) * 3.0), batch, **kw)
        res = {"loss": out[0][0], "by_image": out[0][1], "stats": out[1]}
        if nic:
            res["dfeats"] = out[2]
        return res
    dfe = xe_backward_dlogits(h, randn((n_tok, V), 21) * 0.01, grads, **kw)
    return {"dfeats": dfe} if nic else {}


os.makedirs(OUT, exist_ok=True)
files = 0
for family in ("butd", "aoa", "nic"):
    h, feats, V = make(family)
    for what in ("sample", "sample_n", "rollouts", "xe", "xe_n"):
        if what == "xe_n" and family != "butd":
            continue
        for entry in (ROLLOUT_ENTRIES if what in ("sample", "sample_n", "rollouts") else XE_ENTRIES):
            if (entry == "sample_backward_dlogp" and family != "butd") or (what == "xe_n" and entry != "xe_backward"):
                continue
            rows = store(h, feats, V, what)
            grads = h.new_grads()
            outs = backward(h, entry, rows, sum(LENGTHS_N) if what == "xe_n" else sum(LENGTHS), V, grads)
            torch.cuda.synchronize()
            for name, t in list(outs.items()) + [("grad." + k, v) for k, v in grads.items()]:
                np.save(os.path.join(OUT, "%s.%s.%s.%s.npy" % (family, what, entry, name)), t.detach().cpu().numpy())
                files += 1
    h.close()
print(json.dumps({"device": torch.cuda.get_device_name(0), "dir": OUT, "files": files}))
