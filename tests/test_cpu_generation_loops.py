"""The batch loops of engine.py on the CPU (no GPU, no library call): the ten caption-generation and scoring entry points -- greedy /
beam evaluation, sampling, constrained search, sampling without replacement and scoring, each for one model and for an ensemble --
and the two XE epochs, run on stand-ins.  An engine subclass puts the image ids into its "features", a fake handle derives its
tokens from them, and EnsembleHandle, stochastic_beam.sample_distinct, constrained.beam_search, scoring.score_captions and the two
distillation calls are replaced by recorders.  What is pinned: the exact JSON, every handle call with its arguments, the sharding
over ranks and the gathered order, the reuse of the ensemble handle, the chunking of a batch above the row capacity, the bit-exact
trip of the scores through the gather, and the call sequence of an XE step."""
import contextlib
import types

import numpy as np
import pytest
import torch

from simpleimagecaptionzoo_amd import constrained, dist, distill, engine, ensemble, scoring, stochastic_beam
from simpleimagecaptionzoo_amd.regions import RegionBatch
from simpleimagecaptionzoo_amd.vocab import synthetic_vocab

VOCAB = synthetic_vocab(40)
BATCHES = ([11, 12], [13], [14, 15, 16])          # unequal batches: 2, 1, 3 images
IDS = [i for b in BATCHES for i in b]
EMPTY = {13, 1313}                               # the image (alone / under the ensemble) whose second distinct slot is unoccupied


def W(i):
    return VOCAB.ix2word[i]


def A(v):
    return 4 + v % 30


def B(v):
    return 4 + (v // 7) % 30


# ---- what the fake decoders return for an image whose feature value is v --------------------------------------------------------
def greedy_row(v, max_len):
    return [A(v), 0, B(v), 2] + [5] * (max_len - 4)


def beam_row(v, shift):
    return [1, A(v) + shift, 0, B(v), 2][:3 + v % 3]


def sample_row(v, j, max_len):
    return ([A(v), 0, B(v), 2] if j % 2 == 0 else [B(v), A(v), 2]) + [0] * (max_len - (4 if j % 2 == 0 else 3))


def sample_score(v, j):
    return np.float32(-0.37 * v - j)


def distinct_phi(v, j):
    return np.float32(-0.11 * v - j)


def distinct_g(v, j):
    return np.float64(-v / 3.0 - j / 7.0)


def sat_of(v):
    return (v // 2) % 4


def words_until_end(row, stop_at_pad=False):
    out = []
    for t in row:
        if t == 2 or (stop_at_pad and t == 0):
            break
        if t != 1:
            out.append(W(t))
    return " ".join(out)


def desc(f):
    """the features a call received, as plain values"""
    if isinstance(f, list):
        return [desc(x) for x in f]
    if isinstance(f, RegionBatch):
        return ("RB", [int(x) for x in f.feats[:, 0, 0]], list(f.counts))
    return [int(x) for x in f[:, 0]]


def one_vals(f):
    d = desc(f)
    return d[1] if isinstance(d, tuple) else d


class _Decoder:
    """the decode calls of a handle on CPU tensors; `_vals` turns the features into one value per image"""
    V = len(VOCAB)

    def greedy(self, feats, max_len):
        self.log.append(("greedy", self.name, desc(feats), max_len))
        return torch.tensor([greedy_row(v, max_len) for v in self._vals(feats)], dtype=torch.int64)

    def _beam(self, feats, shift):
        vals = self._vals(feats)
        seqs, lens = torch.zeros(len(vals), 51), torch.zeros(len(vals), dtype=torch.int32)
        for i, v in enumerate(vals):
            row = beam_row(v, shift)
            seqs[i, :len(row)] = torch.tensor(row, dtype=torch.float32)
            lens[i] = len(row)
        return seqs, lens

    def beam_search(self, feats, beam, max_steps):
        self.log.append(("beam_search", self.name, desc(feats), beam, max_steps))
        return self._beam(feats, 0)

    def beam_search_opts(self, feats, beam, max_steps, n_best, lp, ngram, groups, diversity):
        self.log.append(("beam_search_opts", self.name, desc(feats), beam, max_steps, n_best, lp, ngram, groups, diversity))
        seqs, lens = self._beam(feats, 1)
        return seqs[:, None], lens[:, None], torch.zeros(len(lens), 1)

    def sample_decode(self, feats, n, max_len, temperature, top_k, top_p, seed):
        self.log.append(("sample_decode", self.name, desc(feats), n, max_len, temperature, top_k, top_p, seed))
        vals = self._vals(feats)
        ids = torch.tensor([sample_row(v, j, max_len) for v in vals for j in range(n)], dtype=torch.int64)
        score = torch.from_numpy(np.array([sample_score(v, j) for v in vals for j in range(n)], dtype=np.float32))
        return ids, None, score


class _Handle(_Decoder):
    def __init__(self, name, log, max_rows):
        self.name, self.log, self.max_rows = name, log, max_rows

    def _vals(self, feats):
        return one_vals(feats)


class _Ens(_Decoder):
    """stands in for ensemble.EnsembleHandle"""
    built = []
    name = "ens"

    def __init__(self, handles, weights=None):
        self.handles, self.weights = list(handles), weights
        self.log = self.handles[0].log
        self.max_rows = min(h.max_rows for h in self.handles)
        _Ens.built.append(self)

    def _vals(self, feats):
        assert isinstance(feats, list) and len(feats) == len(self.handles)
        return [sum(vs) for vs in zip(*[one_vals(f) for f in feats])]


class _Model:
    scheduled_sampling, ss_prob = False, 0.0

    def __init__(self, eng):
        self.eng = eng

    def eval(self):
        self.eng.mode = "eval"

    def train(self):
        self.eng.mode = "train"

    def _handle(self):
        self.eng.log.append(("_handle", self.eng.name))
        return self.eng.handle

    def _next_rng(self):
        self.eng.log.append(("_next_rng", self.eng.name))
        return "rng-next"


class _Eng(engine.BUTDDetection_Eng):
    """An engine without a device: features = the image ids times `scale` (so that two members differ), as a [B, 1] tensor or, with
    `regions`, a RegionBatch of [B, 2, 1] with per-image counts id % 3 + 1."""

    def __init__(self, name, log, scale=1, max_rows=64, regions=False, fresh_handle_from=None):
        self.name, self.log, self.scale, self.regions = name, log, scale, regions
        self.caption_vocab, self.device = VOCAB, torch.device("cpu")
        self.model, self.mode = _Model(self), None
        self.handle = _Handle(name, log, max_rows)
        self.fresh_handle_from, self.second = fresh_handle_from, _Handle(name, log, max_rows)
        self.n_modify = self.n_features = self.n_hot = 0
        self.feats_made = []
        self.last_distill_terms = None

    def modify_visual_inputs(self, img_tensors, supp_info_datas=None):
        self.n_modify += 1
        return {"ids": supp_info_datas["ids"]}

    def _features(self, visual_inputs):
        self.n_features += 1
        assert self.mode is not None
        ids = torch.tensor(visual_inputs["ids"], dtype=torch.float32) * self.scale
        f = ids[:, None]
        if self.regions:
            f = RegionBatch(ids[:, None, None].repeat(1, 2, 1), [int(i) % 3 + 1 for i in visual_inputs["ids"]])
        self.feats_made.append(f)
        return f

    def _hot_handle(self):
        self.n_hot += 1
        assert self.mode == "eval"
        if self.fresh_handle_from is not None and self.n_hot > self.fresh_handle_from:
            return self.second
        return self.handle

    # the training step's engine-side calls, recorded
    def _grads(self):
        self.log.append(("_grads",))
        return "grads"

    def _xe_token_norm(self, h, lengths):
        self.log.append(("_xe_token_norm", lengths))
        return 7.0

    def _reduce_grads_begin(self, h):
        self.log.append(("reduce_begin",))
        return "ov"

    def _reduce_grads_end(self, overlapped):
        self.log.append(("reduce_end", overlapped))

    def _apply(self, optimizer, clip):
        self.log.append(("_apply", optimizer, clip))


class _Loader:
    """indexable (so that _rank_batches asks for a rank's own batches only); records which batches were asked for"""

    def __init__(self, batches=BATCHES, scst=False):
        self.batches, self.asked, self.scst = batches, [], scst

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        if i >= len(self.batches):
            raise IndexError(i)
        self.asked.append(i)
        ids = self.batches[i]
        if self.scst:
            return tuple(ids), None, self.scst, {"ids": list(ids)}
        return tuple(ids), None, {"ids": list(ids)}


class _Log(list):
    """the recorded calls; `feats` holds the feature objects sample_distinct received (for identity checks)"""

    def __init__(self):
        super().__init__()
        self.feats = []


@pytest.fixture
def log(monkeypatch):
    log = _Log()
    _Ens.built = []
    monkeypatch.setattr(engine, "_on_stream", lambda eng: contextlib.nullcontext())
    monkeypatch.setattr(ensemble, "EnsembleHandle", _Ens)

    def sample_distinct(h, feats, n, max_len, temperature, rng):
        log.append(("sample_distinct", h.name, desc(feats), n, max_len, temperature, rng))
        log.feats.append(feats)
        vals = h._vals(feats)
        rows = [(v, j) for v in vals for j in range(n)]
        gone = [v in EMPTY and j == 1 for v, j in rows]
        ids = torch.tensor([[0] * max_len if g else sample_row(v, j, max_len) for (v, j), g in zip(rows, gone)], dtype=torch.int64)
        lens = torch.tensor([0 if g else 4 - j % 2 for (v, j), g in zip(rows, gone)], dtype=torch.int32)
        phi = torch.from_numpy(np.array([-np.inf if g else distinct_phi(v, j) for (v, j), g in zip(rows, gone)], dtype=np.float32))
        G = torch.from_numpy(np.array([-np.inf if g else distinct_g(v, j) for (v, j), g in zip(rows, gone)], dtype=np.float64))
        return ids, lens, torch.ones_like(lens), phi, G

    def beam_search(h, feats, words, beam, max_steps, n_best, lp, ngram):
        log.append(("constrained", h.name, desc(feats), np.asarray(words).tolist(), beam, max_steps, n_best, lp, ngram))
        vals = h._vals(feats)
        assert len(vals) == len(words)
        seqs, lens = h._beam(feats, 0)
        return seqs[:, None], lens[:, None], torch.zeros(len(vals), 1), torch.tensor([[sat_of(v)] for v in vals], dtype=torch.int32)

    def score_captions(h, feats, ids, n):
        log.append(("score", h.name, desc(feats), np.asarray(ids).tolist(), n))
        vals = h._vals(feats)
        assert len(vals) * n == len(ids)
        logp = -(np.repeat(np.array(vals, dtype=np.float32), n)[:, None] + ids.astype(np.float32) / 64)
        logp[ids == 0] = 0
        return torch.from_numpy(logp), torch.from_numpy(logp.sum(1))

    monkeypatch.setattr(stochastic_beam, "sample_distinct", sample_distinct)
    monkeypatch.setattr(constrained, "beam_search", beam_search)
    monkeypatch.setattr(scoring, "score_captions", score_captions)
    return log


def single(log, **kw):
    return [_Eng("A", log, **kw)]


def pair(log, **kw):
    return [_Eng("A", log, **kw), _Eng("B", log, scale=100, **kw)]


def member_feats(engines, ids):
    """what the recorder sees as the features of images `ids`: one list for a model, a list of one per member for an ensemble"""
    per = [[i * e.scale for i in ids] for e in engines]
    return per if len(engines) > 1 else per[0]


def value(engines, i):
    return sum(i * e.scale for e in engines)


def who(engines):
    return "ens" if len(engines) > 1 else "A"


def each_engine_prepared_every_batch_once(engines, n_batches=len(BATCHES)):
    for e in engines:
        assert (e.n_modify, e.n_features, e.n_hot, e.mode) == (n_batches, n_batches, n_batches, "eval"), e.name


# ---- the entry points, single model (m = 1) and ensemble of two (m = 2) ----------------------------------------------------------
def run_eval(engines, loader, beam=-1, **opts):
    if len(engines) == 1:
        return engines[0].eval_captions_json_generation(loader, beam, False, **opts)
    return engine.eval_ensemble_captions_json_generation(engines, loader, beam, False, **opts)


def run_sample(engines, loader, n=2, seed=3):
    if len(engines) == 1:
        return engines[0].sample_captions_json_generation(loader, n, 0.7, 5, 0.9, seed, False)
    return engine.sample_ensemble_captions_json_generation(engines, loader, n, 0.7, 5, 0.9, seed, False)


CONSTRAINTS = {14: ["w3", "zzz"], 16: [["w4", "w5"]]}            # "zzz" is out of the vocabulary: dropped, reported unsatisfied


def run_constrained(engines, loader, constraints=CONSTRAINTS, beam=3):
    if len(engines) == 1:
        return engines[0].constrained_captions_json_generation(loader, constraints, beam, False, length_penalty="avg_0.5", block_ngram=2)
    return engine.constrained_ensemble_captions_json_generation(engines, loader, constraints, beam, False, length_penalty="avg_0.5",
                                                                block_ngram=2)


def run_distinct(engines, loader, n=2, seed=3):
    if len(engines) == 1:
        return engines[0].sample_distinct_captions_json_generation(loader, n, 0.7, seed, False)
    return engine.sample_distinct_ensemble_captions_json_generation(engines, loader, n, 0.7, seed, False)


ENTRIES = [{"image_id": i, "caption": c, "tag": "%d%s" % (i, c)} for i in IDS for c in ("w%d w2" % (i - 10), "w1")]


def run_score(engines, loader, entries=ENTRIES, n=2):
    if len(engines) == 1:
        return engines[0].score_captions_json(loader, entries, n, False)
    return engine.score_ensemble_captions_json(engines, loader, entries, n, False)


MAKERS = {1: single, 2: pair}


@pytest.mark.parametrize("m", [1, 2])
def test_greedy_evaluation(m, log, capsys):
    engines, loader = MAKERS[m](log), _Loader()
    got = run_eval(engines, loader)
    assert got == [{"image_id": i, "caption": "%s <pad> %s" % (W(A(value(engines, i))), W(B(value(engines, i))))} for i in IDS]
    assert got[0] == {"image_id": 11, "caption": ("w11 <pad> w1", "w1 <pad> w8")[m - 1]}         # 11 / 1111: spelled out once
    assert list(log) == [("greedy", who(engines), member_feats(engines, b), 20) for b in BATCHES]
    assert loader.asked == [0, 1, 2]
    each_engine_prepared_every_batch_once(engines)
    want = "Generating captions json for evaluation. Beam Search: False\n" if m == 1 else \
        "Generating captions json for evaluation (ensemble of 2). Beam Search: False\n"
    assert capsys.readouterr().out == want


@pytest.mark.parametrize("m", [1, 2])
def test_beam_evaluation_without_and_with_options(m, log, capsys):
    engines = MAKERS[m](log)
    got = run_eval(engines, _Loader(), 4)
    shift = 0 if m == 1 else 1                   # one model without options: beam_search; the ensemble: always beam_search_opts
    assert got == [{"image_id": i, "caption": words_until_end(beam_row(value(engines, i), shift))} for i in IDS]
    if m == 1:
        assert list(log) == [("beam_search", "A", member_feats(engines, b), 4, 50) for b in BATCHES]
    else:
        assert list(log) == [("beam_search_opts", "ens", member_feats(engines, b), 4, 50, 1, None, 0, 1, 0.0) for b in BATCHES]
    assert "Beam Search: True" in capsys.readouterr().out
    del log[:]
    got = run_eval(engines, _Loader(), 4, length_penalty=("wu", 0.6), block_ngram=3, beam_groups=2, diversity=0.5)
    assert got == [{"image_id": i, "caption": words_until_end(beam_row(value(engines, i), 1))} for i in IDS]
    assert list(log) == [("beam_search_opts", who(engines), member_feats(engines, b), 4, 50, 1, ("wu", 0.6), 3, 2, 0.5) for b in BATCHES]
    # an evaluation row does not stop at <pad>: the longest rows read on past the 0 up to <end>
    assert any(" <pad> w" in e["caption"] for e in got) and any(e["caption"].endswith("<pad>") for e in got)


def sampled(engines, ids=IDS, n=2):
    return [{"image_id": i, "caption": words_until_end(sample_row(value(engines, i), j, 20), True),
             "score": float(sample_score(value(engines, i), j))} for i in ids for j in range(n)]


@pytest.mark.parametrize("m", [1, 2])
def test_sampling(m, log):
    engines, loader = MAKERS[m](log), _Loader()
    got = run_sample(engines, loader)
    assert got == sampled(engines)
    # a sampled row with a 0 before <end> prints up to the 0; the float32 score comes back bit for bit
    assert got[0]["caption"] == W(A(value(engines, 11))) and got[1]["caption"].count(" ") == 1
    assert np.float32(got[3]["score"]) == sample_score(value(engines, 12), 1) and got[3]["score"] < 0
    assert list(log) == [("sample_decode", who(engines), member_feats(engines, b), 2, 20, 0.7, 5, 0.9, (3 << 20) + k)
                         for k, b in enumerate(BATCHES)]
    each_engine_prepared_every_batch_once(engines)


def constrained_entries(engines, ids=IDS):
    out = []
    for i in ids:
        v = value(engines, i)
        flags = {14: [bool(sat_of(v) & 1), False], 16: [bool(sat_of(v) & 1)]}.get(i, [])
        out.append({"image_id": i, "caption": words_until_end(beam_row(v, 0)), "satisfied": flags})
    return out


@pytest.mark.parametrize("m", [1, 2])
def test_constrained_search(m, log):
    engines = MAKERS[m](log)
    got = run_constrained(engines, _Loader())
    assert got == constrained_entries(engines)
    assert got[3]["satisfied"] == [True, False] and got[5]["satisfied"] == [False]
    none = lambda k: [[] for _ in range(k)]      # noqa: E731    (no constraint in the batch: words [k, 0, 1])
    assert list(log) == [
        ("constrained", who(engines), member_feats(engines, [11, 12]), none(2), 3, 50, 1, "avg_0.5", 2),
        ("constrained", who(engines), member_feats(engines, [13]), none(1), 3, 50, 1, "avg_0.5", 2),
        ("constrained", who(engines), member_feats(engines, [14, 15, 16]), [[[7, -1]], [[-1, -1]], [[8, 9]]], 3, 50, 1, "avg_0.5", 2)]
    each_engine_prepared_every_batch_once(engines)


def distinct_entries(engines, ids=IDS, n=2):
    out = []
    for i in ids:
        v = value(engines, i)
        for j in range(n):
            if not (v in EMPTY and j == 1):
                out.append({"image_id": i, "caption": words_until_end(sample_row(v, j, 20), True), "score": float(distinct_phi(v, j)),
                            "perturbed": float(distinct_g(v, j))})
    return out


@pytest.mark.parametrize("m", [1, 2])
def test_sampling_without_replacement(m, log):
    engines = MAKERS[m](log)
    got = run_distinct(engines, _Loader())
    assert got == distinct_entries(engines)
    # the slot with lens == 0 is dropped and its neighbours stay where they are; float32 / float64 come back bit for bit
    assert [e["image_id"] for e in got] == [11, 11, 12, 12, 13, 14, 14, 15, 15, 16, 16]
    assert got[4]["perturbed"] == float(distinct_g(value(engines, 13), 0)) and np.float32(got[4]["score"]) == distinct_phi(value(engines, 13), 0)
    assert got[5]["perturbed"] == float(distinct_g(value(engines, 14), 0)) and got[5]["perturbed"] != float(np.float32(got[5]["perturbed"]))
    assert list(log) == [("sample_distinct", who(engines), member_feats(engines, b), 2, 20, 0.7, ((3 << 20) + k, 0)) for k, b in enumerate(BATCHES)]
    # a batch that fits is handed over unsliced: the very objects the engines made
    for k in range(len(BATCHES)):
        made = [e.feats_made[k] for e in engines]
        assert all(a is b for a, b in zip(log.feats[k], made)) if m == 2 else log.feats[k] is made[0]
    each_engine_prepared_every_batch_once(engines)


def scored_entries(engines, entries=ENTRIES):
    out = []
    for e in entries:
        ids = [VOCAB(w) for w in e["caption"].split()] + [2]
        lp = [float(-np.float32(np.float32(value(engines, e["image_id"])) + np.float32(t) / 64)) for t in ids]
        out.append(dict(e, logprob=float(np.sum(np.array(lp, dtype=np.float32), dtype=np.float32)), tokens=len(ids), logprobs=lp))
    return out


@pytest.mark.parametrize("m", [1, 2])
def test_scoring_given_captions(m, log):
    engines, loader = MAKERS[m](log), _Loader()
    got = run_score(engines, loader)
    assert got == scored_entries(engines)
    assert got[0]["tokens"] == 3 and got[1]["tokens"] == 2 and got[0]["tag"] == "11w1 w2"
    at = 0
    for call, b in zip(log, BATCHES):
        ids = scoring.encode_captions([e["caption"] for e in ENTRIES[at:at + 2 * len(b)]], VOCAB)
        assert call == ("score", who(engines), member_feats(engines, b), ids.tolist(), 2)
        at += 2 * len(b)
    assert len(log) == 3 and loader.asked == [0, 1, 2]
    each_engine_prepared_every_batch_once(engines)


def test_reference_perplexity_scores_in_groups_of_eight_and_prepares_the_batch_for_each(log):
    gts = {i: ["w1 w2"] * (9 if i == 12 else 2) for i in IDS}
    eng = single(log)[0]
    got = eng.reference_perplexity(_Loader(scst=gts), False)
    assert got["captions"] == 2 * 5 + 9 and got["tokens"] == 3 * got["captions"]
    assert [(c[2], len(c[3]), c[4]) for c in log] == [([11, 12], 16, 8), ([11, 12], 2, 1), ([13], 2, 2), ([14, 15, 16], 6, 2)]
    assert (eng.n_modify, eng.n_features, eng.n_hot) == (4, 4, 4)


# ---- sharding over two ranks -----------------------------------------------------------------------------------------------------
class _World:
    """dist as two ranks run in turn: gather_caption_rows merges what every rank has handed it so far, packed as the real one packs"""

    def __init__(self, monkeypatch):
        self.rank, self.packs = 0, []
        monkeypatch.setattr(dist, "is_distributed", lambda: True)
        monkeypatch.setattr(dist, "rank", lambda: self.rank)
        monkeypatch.setattr(dist, "world_size", lambda: 2)
        monkeypatch.setattr(dist, "gather_caption_rows", self.gather)

    def gather(self, keys, image_ids, rows, device, width=52):
        assert device == torch.device("cpu")
        pack = np.full((len(rows), 2 + width), -1, dtype=np.int64)
        for j, r in enumerate(rows):
            pack[j, 0], pack[j, 1] = keys[j], image_ids[j]
            pack[j, 2:2 + len(r)] = np.asarray(r, dtype=np.int64)
        self.packs.append(pack)
        allp = np.concatenate(self.packs)
        allp = allp[np.argsort(allp[:, 0], kind="stable")]
        return [int(x) for x in allp[:, 1]], [row[2:][row[2:] >= 0] for row in allp]


SHARDED = {"greedy": lambda e, l: run_eval(e, l), "beam": lambda e, l: run_eval(e, l, 4), "beam_opts": lambda e, l: run_eval(e, l, 4, block_ngram=2),
           "sample": run_sample, "constrained": run_constrained, "distinct": run_distinct}


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("path", sorted(SHARDED))
def test_two_ranks_decode_their_own_batches_and_gather_the_unsharded_list(path, m, log, monkeypatch):
    run = SHARDED[path]
    whole = run(MAKERS[m](log), _Loader())
    calls = list(log)
    del log[:]
    world = _World(monkeypatch)
    asked, sharded = [], None
    for rank in (0, 1):
        world.rank = rank
        engines, loader = MAKERS[m](log), _Loader()
        sharded = run(engines, loader)
        asked.append(loader.asked)
        each_engine_prepared_every_batch_once(engines, len(loader.asked))
    assert asked == [[0, 2], [1]]                            # each rank asked the loader for its own batches only
    assert sharded == whole                                  # the last rank's gather holds every rank's rows, in loader order
    assert sorted(log, key=repr) == sorted(calls, key=repr) and list(log) == [calls[0], calls[2], calls[1]]
    if path == "distinct":                                   # the dropped slot's key is consumed: image 13's only row has key (1 << 20) + 0
        keys = [int(k) for p in world.packs for k in p[:, 0]]
        assert sorted(keys) == [(b << 20) + r for b, rows in enumerate((4, 2, 6)) for r in range(rows) if (b, r) != (1, 1)]
    else:
        per = 2 if path == "sample" else 1
        assert sorted(int(k) for p in world.packs for k in p[:, 0]) == [(b << 20) + r for b, ids in enumerate(BATCHES) for r in range(per * len(ids))]


@pytest.mark.parametrize("m", [1, 2])
def test_scoring_is_not_sharded(m, log, monkeypatch):
    whole = run_score(MAKERS[m](log), _Loader())
    world = _World(monkeypatch)
    for rank in (0, 1):
        world.rank = rank
        loader = _Loader()
        assert run_score(MAKERS[m](log), loader) == whole and loader.asked == [0, 1, 2]
    assert world.packs == []


# ---- the ensemble handle --------------------------------------------------------------------------------------------------------
ENSEMBLE_RUNS = {"greedy": lambda e, l: run_eval(e, l), "sample": run_sample, "constrained": run_constrained, "distinct": run_distinct,
                 "score": run_score}


@pytest.mark.parametrize("path", sorted(ENSEMBLE_RUNS))
def test_ensemble_handle_is_kept_while_the_members_are_and_rebuilt_when_one_changes(path, log):
    engines = pair(log)
    engine_weights = [0.25, 0.75]
    run = ENSEMBLE_RUNS[path]
    run(engines, _Loader())
    assert len(_Ens.built) == 1 and _Ens.built[0].handles == [engines[0].handle, engines[1].handle] and _Ens.built[0].weights is None
    _Ens.built = []
    engines = [_Eng("A", log), _Eng("B", log, scale=100, fresh_handle_from=1)]          # B hands out a new handle from the second batch on
    if path == "greedy":
        engine.eval_ensemble_captions_json_generation(engines, _Loader(), -1, False, weights=engine_weights)
    else:
        run(engines, _Loader())
    assert len(_Ens.built) == 2
    assert _Ens.built[0].handles[1] is engines[1].handle and _Ens.built[1].handles[1] is engines[1].second
    assert all(b.handles[0] is engines[0].handle for b in _Ens.built)
    if path == "greedy":
        assert all(b.weights is engine_weights for b in _Ens.built)


@pytest.mark.parametrize("path", ["greedy", "sample"])
def test_single_model_paths_build_no_ensemble_handle(path, log):
    ENSEMBLE_RUNS[path](single(log), _Loader())
    run_constrained(single(log), _Loader())
    run_distinct(single(log), _Loader())
    run_score(single(log), _Loader())
    assert _Ens.built == []


# ---- chunking a batch above the row capacity ------------------------------------------------------------------------------------
def seen_feats(engines, regions, ids):
    return ("RB", ids, [i % 3 + 1 for i in ids]) if regions else member_feats(engines, ids)


def chunks_of(log, kind):
    return [c[2] for c in log if c[0] == kind]


@pytest.mark.parametrize("m, regions", [(1, False), (1, True), (2, False)])
def test_constrained_chunks_tile_the_batch(m, regions, log):
    engines = MAKERS[m](log, max_rows=12, regions=regions)          # batch 3 holds a constraint: 2 * 3 rows per image, 2 images per call
    got = run_constrained(engines, _Loader())
    assert got == constrained_entries(engines)
    sl = lambda ids: seen_feats(engines, regions, ids)      # noqa: E731
    assert chunks_of(log, "constrained") == [sl([11, 12]), sl([13]), sl([14, 15]), sl([16])]
    assert [c[3] for c in log][2:] == [[[[7, -1]], [[-1, -1]]], [[[8, 9]]]]                  # the constraints are sliced with the features


def test_constrained_max_chunk_and_refusal(log):
    eng = single(log)[0]
    got = engine._constrained_captions_json_generation([eng], None, False, _Loader(), {}, 3, False, None, 0, max_chunk=1)
    assert got == [{"image_id": i, "caption": words_until_end(beam_row(i, 0)), "satisfied": []} for i in IDS]
    assert chunks_of(log, "constrained") == [[i] for i in IDS]
    del log[:]
    engine._constrained_captions_json_generation([eng], None, False, _Loader(), {}, 3, False, None, 0, max_chunk=5)      # above `per`: no effect
    assert chunks_of(log, "constrained") == [list(b) for b in BATCHES]
    for engines in (single(log, max_rows=2), pair(log, max_rows=2)):
        with pytest.raises(ValueError, match="^one image takes 3 rows, the handle's row capacity is 2$"):
            run_constrained(engines, _Loader(), {})


@pytest.mark.parametrize("m, regions", [(1, False), (1, True), (2, False)])
def test_scoring_chunks_tile_the_batch(m, regions, log):
    engines = MAKERS[m](log, max_rows=5, regions=regions)            # 5 // 2 captions: 2 images per call
    got = run_score(engines, _Loader())
    assert got == scored_entries(engines)
    sl = lambda ids: seen_feats(engines, regions, ids)      # noqa: E731
    assert chunks_of(log, "score") == [sl([11, 12]), sl([13]), sl([14, 15]), sl([16])]
    assert [len(c[3]) for c in log] == [4, 2, 4, 2]
    for engines in (single(log, max_rows=1), pair(log, max_rows=1)):
        with pytest.raises(ValueError, match="^2 captions per image exceed the handle's row capacity 1$"):
            run_score(engines, _Loader())


@pytest.mark.parametrize("m, regions", [(1, False), (1, True), (2, False)])
def test_distinct_chunks_tile_the_batch_and_carry_their_offset_into_the_seed(m, regions, log):
    engines = MAKERS[m](log, max_rows=5, regions=regions)            # 5 // 2 hypotheses: 2 images per call
    got = run_distinct(engines, _Loader())
    assert got == distinct_entries(engines)
    sl = lambda ids: seen_feats(engines, regions, ids)      # noqa: E731
    assert chunks_of(log, "sample_distinct") == [sl([11, 12]), sl([13]), sl([14, 15]), sl([16])]
    assert [c[6] for c in log] == [((3 << 20) + 0, 0), ((3 << 20) + 1, 0), ((3 << 20) + 2, 0), ((3 << 20) + 2, 2)]
    assert log.feats[0] is engines[0].feats_made[0] or m == 2        # a batch that fits: unsliced
    del log[:]
    engines = MAKERS[m](log, max_rows=1)                             # not even one image fits: clamped to one image per call, no error
    assert run_distinct(engines, _Loader()) == distinct_entries(engines)
    assert chunks_of(log, "sample_distinct") == [member_feats(engines, [i]) for i in IDS]
    assert [c[6] for c in log] == [((3 << 20) + k, lo) for k, b in enumerate(BATCHES) for lo in range(len(b))]


# ---- the XE epochs --------------------------------------------------------------------------------------------------------------
class _TrainHandle:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def xe_forward(self, feats, captions, lengths, rng, train=False, want_logits=False):
        self.log.append(("xe_forward", self.name, desc(feats), captions, lengths, rng, train))

    def xe_backward(self, grads, smoothing, n_glob):
        self.log.append(("xe_backward", self.name, grads, smoothing, n_glob))
        return torch.tensor([1.5])


def train_loader():
    return [((11, 12), None, "caps0", [5, 4], {"ids": [11, 12]}), ((13,), None, "caps1", [3], {"ids": [13]})]


def step_around(backward, ids, caps, lengths, rng):
    rng_call = [] if rng != "rng-next" else [("_next_rng", "S")]
    return [("_handle", "S")] + rng_call + [("xe_forward", "S", ids, caps, lengths, rng, True), ("_grads",), ("_xe_token_norm", lengths),
                                            ("reduce_begin",), backward, ("reduce_end", "ov"), ("_apply", "opt", 0.1)]


@pytest.mark.parametrize("rngs", [None, ["r0", "r1"]])
def test_training_and_distillation_epochs_issue_the_same_step_around_their_backward_call(rngs, log, monkeypatch):
    crit = types.SimpleNamespace(smoothing=0.2)
    student = _Eng("S", log)
    student.handle = _TrainHandle("S", log)
    losses = student.training_epoch(train_loader(), "opt", crit, False, rngs)
    assert [float(x) for x in losses] == [1.5, 1.5] and student.mode == "train" and (student.n_modify, student.n_features) == (2, 2)
    rng = lambda k: rngs[k] if rngs else "rng-next"      # noqa: E731
    plain = ("xe_backward", "S", "grads", 0.2, 7.0)
    want = step_around(plain, [11, 12], "caps0", [4, 3], rng(0)) + step_around(plain, [13], "caps1", [2], rng(1))
    assert list(log) == want
    del log[:]

    def teacher_logits(handles, feats_list, captions, lengths):
        log.append(("teacher_logits", [h.name for h in handles], desc(list(feats_list)), captions, lengths))
        return "t_logits"

    def xe_backward_distill(h, grads, t_logits, weights, alpha, temperature, smoothing, n_glob):
        log.append(("xe_backward_distill", h.name, grads, t_logits, weights, alpha, temperature, smoothing, n_glob))
        return torch.tensor([2.5]), "hard", "kd"
    monkeypatch.setattr(distill, "teacher_logits", teacher_logits)
    monkeypatch.setattr(distill, "xe_backward_distill", xe_backward_distill)
    student = _Eng("S", log)
    student.handle = _TrainHandle("S", log)
    teachers = [_Eng("T1", log, scale=10), _Eng("T2", log, scale=100)]
    for t in teachers:
        t.handle = _TrainHandle(t.name, log)
    losses = student.distill_training_epoch(train_loader(), "opt", crit, teachers, False, rngs, alpha=0.3, temperature=2.0, weights=[1.0, 3.0])
    assert [float(x) for x in losses] == [2.5, 2.5] and student.last_distill_terms == [("hard", "kd")] * 2
    assert student.mode == "train" and [t.mode for t in teachers] == ["eval", "eval"]
    assert [(e.n_modify, e.n_features) for e in [student] + teachers] == [(2, 2)] * 3
    dist_bw = ("xe_backward_distill", "S", "grads", "t_logits", [1.0, 3.0], 0.3, 2.0, 0.2, 7.0)

    def teachers_first(ids, caps, lengths):
        return [("_handle", "T1"), ("_handle", "T2"), ("teacher_logits", ["T1", "T2"], [[10 * i for i in ids], [100 * i for i in ids]], caps, lengths)]
    assert list(log) == teachers_first([11, 12], "caps0", [4, 3]) + step_around(dist_bw, [11, 12], "caps0", [4, 3], rng(0)) \
        + teachers_first([13], "caps1", [2]) + step_around(dist_bw, [13], "caps1", [2], rng(1))
