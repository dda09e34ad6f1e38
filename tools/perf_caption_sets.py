"""Consensus reranking of caption sets, device against host: N synthetic images x K candidates of about 10 words (a reference of
the image with up to three words replaced) x 5 references, df table over the N images' references.
  device leg: caption strings -> pack_candidates (host) -> CiderDReward.pairwise (cook on the device + pairwise match + argmax) ->
              `best` copied to the host; wall clock around a synchronising copy, median of R runs after one warm-up.
  oracle leg: the same picks with oracle.ciderd.ciderd_scores on this host's CPU (each candidate against its K - 1 siblings, first
              argmax), median of R runs over the first M images, scaled to N (it is linear in the images).
The picks of the two legs are compared on the M images.  A second device line times the rest of a set report on the same candidates
(scores against the reference store, n-gram counts, mBLEU), store already loaded.
usage: perf_caption_sets.py [N] [K] [R] [M]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from oracle import ciderd as oc
from simpleimagecaptionzoo_amd import caption_sets as cs
from simpleimagecaptionzoo_amd.ciderd import CiderDReward
from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
from simpleimagecaptionzoo_amd.vocab import synthetic_vocab

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 5
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
M = min(N, int(sys.argv[4]) if len(sys.argv) > 4 else 500)
V = 2000
vocab = synthetic_vocab(V)
words = [vocab.ix2word[i] for i in range(V)]
gts = synthetic_references(N, words, seed=0)
dfd = document_frequency(gts)
rng = np.random.RandomState(1)
caps = []
for i in range(N):
    grp = []
    for k in range(K):
        w = gts[i][rng.randint(5)].split()
        for _ in range(rng.randint(0, 4)):
            w[rng.randint(len(w))] = words[4 + rng.randint(V - 4)]
        grp.append(" ".join(w))
    caps.append(grp)
n_words = sum(len(c.split()) for g in caps for c in g)
print("%d images x %d candidates (%.1f words each) x 5 references, df table of %d n-grams"
      % (N, K, n_words / (N * K), len(dfd["document_frequency"])))

scorer = CiderDReward(dfd["document_frequency"], dfd["ref_len"], vocab.word2ix, "cuda:0")
scorer.persistent = True


def device_leg():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cands = cs.pack_candidates(caps, vocab.word2ix, "cuda:0")
    t1 = time.perf_counter()
    _, _, best = scorer.pairwise(cands, K)
    best = best.cpu().numpy()                    # synchronises
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, best


device_leg()
runs = [device_leg() for _ in range(R)]
t_dev = float(np.median([r[0] for r in runs]))
t_pack = float(np.median([r[1] for r in runs]))
best = runs[-1][2]
print("device leg: %.1f ms end to end (host packing %.1f ms, device + copy of best %.1f ms; median of %d, min %.1f max %.1f)"
      % (1e3 * t_dev, 1e3 * t_pack, 1e3 * (t_dev - t_pack), R, 1e3 * min(r[0] for r in runs), 1e3 * max(r[0] for r in runs)))

docfreq = oc.DocFreq(dfd["document_frequency"], dfd["ref_len"])


def oracle_leg():
    t0 = time.perf_counter()
    picks = np.zeros(M, np.int32)
    for i in range(M):
        g = caps[i]
        cons = [oc.ciderd_scores([g[a]], [[g[b] for b in range(K) if b != a]], docfreq)[0] for a in range(K)]
        picks[i] = int(np.argmax(cons))
    return time.perf_counter() - t0, picks


oracle_leg()
oruns = [oracle_leg() for _ in range(R)]
t_or = float(np.median([r[0] for r in oruns]))
same = bool(np.array_equal(oruns[-1][1], best[:M]))
print("oracle leg: %.1f ms for the first %d images (median of %d) = %.1f ms scaled to %d images; picks equal the device's: %s"
      % (1e3 * t_or, M, R, 1e3 * t_or * N / M, N, same))
print("ratio oracle / device: %.1fx" % (t_or * N / M / t_dev))

ids = list(range(N))
scorer.preload(gts)
cands = cs.pack_candidates(caps, vocab.word2ix, "cuda:0")


def report_leg():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc = scorer.scores_csr(cands, K, gts, ids).cpu().numpy()
    counts = cs.ngram_counts(cands)
    mb = cs.mbleu(cands)
    return time.perf_counter() - t0, float(np.mean(sc.max(axis=1))), cs.div_n(counts, 2), mb[3]


report_leg()
rruns = [report_leg() for _ in range(R)]
print("rest of the set report on the device (scores against the store, n-gram counts, mBLEU): %.1f ms (median of %d; oracle CIDEr-D %.4f, "
      "Div_2 %.4f, mBleu_4 %.4f)" % (1e3 * float(np.median([r[0] for r in rruns])), R, rruns[-1][1], rruns[-1][2], rruns[-1][3]))
if not same:
    sys.exit("the device's picks differ from the oracle's")
