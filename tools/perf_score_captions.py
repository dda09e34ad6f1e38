"""Scoring given captions at the benchmark width (R 36, D 2048, H = E = A 1024, V 10 102): 128 images x 5 captions of 8 - 16 words
(+ <end>), BUTD, AoA and a two-member BUTD ensemble.  Three routes, ms per batch and captions/s:
  (a) scoring.score_captions with n = 5: the per-image work once per image;
  (b) scoring.score_captions with n = 1 on the features repeated five times;
  (c) the route that existed before: per image one xe_forward(train=False, want_logits=True) over its five captions sorted by
      length + torch.log_softmax + gather, on the device (no ensemble has this route).
Device events around synchronised work, two warm-up rounds, the routes alternated in one process, median of R rounds.
usage: perf_score_captions.py [R]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle  # noqa: E402
from simpleimagecaptionzoo_amd.scoring import score_captions  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N_IMG, N, V, T = 128, 5, 10102, 17


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def xe_inputs(ids, lens):
    """per image, staged on the device outside the timed region: (captions with <sta> sorted by length, steps, packed targets)"""
    out = []
    for i in range(N_IMG):
        order = sorted(range(N), key=lambda j: -lens[i * N + j])
        caps = torch.ones(N, T + 1, dtype=torch.int64)
        caps[:, 1:] = ids[i * N:(i + 1) * N][order]
        steps = [int(lens[i * N + j]) for j in order]
        caps = caps.cuda()
        tgt = torch.cat([caps[:sum(s > t for s in steps), t + 1] for t in range(steps[0])]).view(-1, 1)
        out.append((caps, steps, tgt))
    return out


def xe_route(h, feats, staged):
    """(c) -> log-probs of the scored tokens, packed per image as xe_forward packs them"""
    out = []
    for i, (caps, steps, tgt) in enumerate(staged):
        logits = h.xe_forward(feats[i:i + 1].expand(N, *feats.shape[1:]).contiguous(), caps, steps, None, train=False, want_logits=True)
        out.append(torch.log_softmax(logits, 1).gather(1, tgt))
    return out


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    lens = rs.randint(9, 18, size=N_IMG * N)                      # 8 - 16 words + <end>
    ids = torch.zeros(N_IMG * N, T, dtype=torch.int64)
    for r, l in enumerate(lens):
        ids[r, :l - 1] = torch.from_numpy(rs.randint(4, V, size=l - 1))
        ids[r, l - 1] = 2
    dev_ids = ids.cuda()
    staged = xe_inputs(ids, lens)
    feats = torch.rand(N_IMG, 36, 2048, device="cuda")
    rep = feats.repeat_interleave(N, 0).contiguous()
    butd = BUTDDetection_Captioner(1024, 1024, 1024, V, max_batch=N_IMG, max_beam=N).cuda()._handle()
    butd2 = BUTDDetection_Captioner(1024, 1024, 1024, V, max_batch=N_IMG, max_beam=N).cuda()._handle()
    aoa = AoADetection_Captioner(V, max_batch=N_IMG, max_beam=N).cuda()._handle()
    ens = EnsembleHandle([butd, butd2])
    legs = []
    for name, h in (("BUTD", butd), ("AoA", aoa)):
        legs.append((name + " (a) n = 5", lambda h=h: score_captions(h, feats, dev_ids, N)))
        legs.append((name + " (b) n = 1, features x 5", lambda h=h: score_captions(h, rep, dev_ids, 1)))
        legs.append((name + " (c) xe_forward per image", lambda h=h: xe_route(h, feats, staged)))
    legs.append(("BUTD x 2 ensemble (a) n = 5", lambda: score_captions(ens, [feats, feats], dev_ids, N)))
    legs.append(("BUTD x 2 ensemble (b) n = 1, features x 5", lambda: score_captions(ens, [rep, rep], dev_ids, 1)))
    times = {name: [] for name, _ in legs}
    for rnd in range(R + 2):
        for name, fn in legs:
            ms, out = timed(fn)
            if rnd >= 2:
                times[name].append(ms)
            if rnd == 0 and name.startswith("BUTD (c)"):          # the routes score the same thing
                a = score_captions(butd, feats, dev_ids, N)[0]
                worst = 0.0
                for i in range(N_IMG):
                    order = sorted(range(N), key=lambda j: -lens[i * N + j])
                    steps = [int(lens[i * N + j]) for j in order]
                    want = torch.cat([a[i * N + torch.tensor(order)[:sum(s > t for s in steps)], t] for t in range(steps[0])])
                    worst = max(worst, float((out[i].view(-1) - want).abs().max()))
                print("BUTD: route (c) against route (a): max difference of a log-prob %.3g" % worst)
    print("%d images x %d captions of 8 - 16 words, %d columns; median of %d rounds after 2 warm-up rounds, routes alternated" % (
        N_IMG, N, T, R))
    for name, _ in legs:
        ms = float(np.median(times[name]))
        print("%-44s %9.2f ms per batch  %9.0f captions/s   (min %.2f, max %.2f)" % (
            name, ms, N_IMG * N / ms * 1e3, min(times[name]), max(times[name])))


if __name__ == "__main__":
    main()
