"""What the BUTD, AoA and NIC families share above libicz: the host-side owner of one decoder handle (DecoderHandle) and the
Captioner over it (CaptionerBase).  A family's module declares its structs, state-dict keys and feature check and keeps the
calls only that family has."""
import ctypes as C
import types

import torch

from . import _lib
from . import beam as _beam
from . import sampling as _sampling
from ._lib import check, lib, ptr, stream_ptr
from .beam import nbest_lists
from .scheduled import ScheduledSamplingState

# the icz_<family>_<name> entries the shared methods call; a family lists the ones only it has in `_own_entries`
_ENTRIES = ("create", "destroy", "bind_params", "refresh_weights", "set_option", "set_grad_callback", "set_scheduled_sampling",
            "set_norm_global", "greedy", "sample", "scst_rollouts", "sample_backward", "xe_forward", "xe_backward", "beam_search",
            "beam_search_opts", "beam_search_diverse", "beam_search_constrained", "sample_decode", "sample_distinct", "score_captions", "xe_backward_distill",
            "sample_backward_objective", "xe_backward_swor")


def grad_args(handle, gs, want_dfeats):
    """The gradient arguments of a backward entry of `handle`'s family: its gradient struct `gs` and, for a NicHandle, the d features
    pointer right behind it (zeros like the stored pass's features with want_dfeats, else null) -> (the arguments, d features or
    None).  IczError for want_dfeats on another family.  A function, as the entry points of distill.py, swor.py and scst_objective.py
    that use it are: the handles keep their public surface."""
    if handle.family != "nic":
        if want_dfeats:
            raise _lib.IczError("want_dfeats: only the NIC decoder returns a gradient for its features")
        return (C.byref(gs),), None
    dfe = torch.zeros_like(handle._live[0]) if want_dfeats else None
    return (C.byref(gs), ptr(dfe)), dfe


class DecoderHandle:
    """Wraps icz_<family>_* for a fixed architecture and row / step capacity.  A subclass declares `family`, `kind` (its member
    kind in icz_ensemble_create), `_Params` (the ctypes struct of parameter pointers) with `_param_keys` (the reference
    state-dict key of each field, in field order), `_make_rng` (its icz_rng maker) and `_feats` (its feature check)."""

    family = kind = _Params = _make_rng = None
    _param_keys = ()
    _frozen_keys = frozenset()   # parameters the reference does not optimise: their gradient buffers may be left out
    _own_entries = ()
    _entry_names = {}            # table name -> name in the library where they differ
    _sample_bufs = False         # sample() writes persistent buffers while graphs are on

    @classmethod
    def _entries(cls):
        """The family's library entries, resolved once per class: name -> function for every entry include/icz.h declares for
        it.  One the family lacks is absent, so the method that needs it raises AttributeError."""
        table = cls.__dict__.get("_table")
        if table is None:
            table = types.SimpleNamespace()
            for name in _ENTRIES + cls._own_entries:
                fn = getattr(lib(), "icz_%s_%s" % (cls.family, cls._entry_names.get(name, name)), None)
                if fn is not None and fn.argtypes is not None:      # declared in _lib.lib()
                    setattr(table, name, fn)
            cls._table = table
        return table

    def _create(self, dims, device, entry="create"):
        """The tail of a subclass's __init__: the fields of its dims struct become attributes (R, D, ..., max_rows, max_len).
        entry: the family's creating entry (BUTD: "create_regions" for a region capacity above 64)."""
        for name, _ in dims._fields_:
            setattr(self, name, getattr(dims, name))
        self.device = torch.device(device)
        self._h = C.c_void_p()
        self._params = None
        self._persistent = False
        self._bufs = {}
        self._e = self._entries()
        with torch.cuda.device(self.device):
            check(getattr(self._e, entry)(C.byref(dims), C.byref(self._h)))

    def close(self):
        if self._h:
            self._e.destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buf(self, name, shape, dtype, keep=True):
        """A zeroed output tensor; with graphs on (and `keep`) the one persistent tensor of that name and shape, which the next
        call overwrites: the library's graph cache keys on output pointers."""
        if not (keep and self._persistent):
            return torch.zeros(shape, dtype=dtype, device=self.device)
        key = (name,) + tuple(shape)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.zeros(shape, dtype=dtype, device=self.device)
        return t

    # ---- parameters ---------------------------------------------------------------------------
    def _struct(self, tensors, what, optional=()):
        st = self._Params()
        for (field, _), key in zip(st._fields_, self._param_keys):
            t = tensors.get(key)
            if t is None:
                if key in optional:
                    continue
                raise KeyError(key)
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise _lib.IczError("%s %s must be a contiguous fp32 CUDA tensor" % (what, key))
            setattr(st, field, t.data_ptr())
        return st

    def bind(self, tensors):
        """tensors: {reference state_dict key: fp32 CUDA tensor}.  The tensors are used in place (no copy) and must stay alive;
        call refresh() after every update."""
        st = self._struct(tensors, "parameter")
        self._params = {k: tensors[k] for k in self._param_keys}
        check(self._e.bind_params(self._h, C.byref(st)))
        self.refresh()

    def refresh(self):
        check(self._e.refresh_weights(self._h, stream_ptr()))

    def new_grads(self):
        """Zeroed gradient buffers, one per optimised parameter (same keys / shapes; AoA: the decoder only, AoA_Model.py:669-674)."""
        return {k: torch.zeros_like(t) for k, t in self._params.items() if k not in self._frozen_keys}

    def _grad_struct(self, grads):
        return self._struct(grads, "gradient buffer", self._frozen_keys)

    # ---- decode and training ------------------------------------------------------------------
    def greedy(self, feats, max_len=20):
        """The decoder's greedy sample() in evaluation mode -> ids (B, max_len) int64."""
        feats = self._feats(feats)
        ids = torch.empty(feats.shape[0], max_len, dtype=torch.int64, device=feats.device)
        check(self._e.greedy(self._h, ptr(feats), feats.shape[0], max_len, ptr(ids), stream_ptr()))
        return ids

    def sample(self, feats, max_len=20, rng=None):
        """The decoder's sample_rl (e.g. BUTD_Model.py:191-234), dropout on -> (seq int64 (B,T), logprobs (B,T))."""
        feats = self._feats(feats)
        B = feats.shape[0]
        rng = rng or self._make_rng(0)
        seq = self._buf("sample_seq", (B, max_len), torch.int64, self._sample_bufs)
        lp = self._buf("sample_lp", (B, max_len), torch.float32, self._sample_bufs)
        check(self._e.sample(self._h, ptr(feats), B, max_len, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()))
        self._live = (feats, rng, seq, lp)
        return seq, lp

    def rollouts(self, feats, max_len=20, rng=None):
        """Greedy baseline (eval mode) + sampled rollout (train mode) of one SCST step (Engine.py:256-262), as two concurrent
        chains on the device.  Returns (greedy_ids, seq, logprobs); identical to greedy() followed by sample()."""
        feats = self._feats(feats)
        B = feats.shape[0]
        rng = rng or self._make_rng(0)
        ids = self._buf("greedy_ids", (B, max_len), torch.int64)
        seq = self._buf("sample_seq", (B, max_len), torch.int64)
        lp = self._buf("sample_lp", (B, max_len), torch.float32)
        check(self._e.scst_rollouts(self._h, ptr(feats), B, max_len, C.byref(rng), ptr(ids), ptr(seq), ptr(lp), stream_ptr()))
        self._live = (feats, rng, seq, lp)
        return ids, seq, lp

    def sample_mask_sum(self):
        """Local sum of the REINFORCE mask (Utils.py:307-309) as a 1-element DEVICE tensor (no host round trip)."""
        seq = self._live[2]
        return ((seq[:, :-1] > 0).sum() + seq.shape[0]).float().view(1)

    def set_mask_sum_global(self, t):
        """DP: hand the all-reduced loss normaliser (mask sum of the rollout / token count of the XE batch) over as a 1-element
        device tensor; then sample_backward(..., mask_sum_global=-1) / xe_backward(..., n_tokens_global=-1)."""
        check(self._e.set_norm_global(self._h, ptr(t), stream_ptr()))

    def sample_backward(self, reward, grads, mask_sum_global=0.0):
        """RewardCriterion + backward (Utils.py:295-317) for the last sample(); fills `grads`; returns
        (loss, local mask sum) as 1-element device tensors."""
        reward = reward.to(device=self.device, dtype=torch.float32).contiguous()
        loss = self._buf("rl_loss", (1,), torch.float32)
        msum = self._buf("rl_msum", (1,), torch.float32)
        gs = self._grad_struct(grads)
        check(self._e.sample_backward(self._h, ptr(reward), C.byref(gs), ptr(loss), ptr(msum), float(mask_sum_global), stream_ptr()))
        return loss, msum

    def xe_forward(self, feats, captions, lengths, rng=None, train=True, want_logits=False):
        """The decoder's forward (e.g. BUTD_Model.py:97-151).  lengths = caption lengths minus one (Engine.py:178),
        sorted descending.  Returns packed logits (sum(lengths), V) if want_logits."""
        feats = self._feats(feats)
        B, L = captions.shape
        captions = captions.to(device=feats.device, dtype=torch.int64).contiguous()
        lens = (C.c_int32 * B)(*[int(x) for x in lengths])
        out = torch.empty(sum(int(x) for x in lengths), self.V, device=feats.device) if want_logits else None
        if train and rng is None:
            rng = self._make_rng(0)
        check(self._e.xe_forward(self._h, ptr(feats), ptr(captions), B, L, lens, C.byref(rng) if rng is not None else None,
                                 1 if train else 0, ptr(out), stream_ptr()))
        self._live = (feats, rng, captions)
        self._xe_tokens = sum(int(x) for x in lengths)      # rows of the packed logits (distill.py checks the teachers' against it)
        return out

    def set_scheduled_sampling(self, ss_prob, gate=None, draw=None):
        """Scheduled sampling for the following xe_forward calls (BUTD_Model.py:120-132, AoA_Model.py:258-270, NIC_Model.py:77-89
        with the decoder's `ss_prob`): gate / draw are optional explicit uniforms [T, B] (parity tests), default Philox."""
        keep = [None if u is None else torch.as_tensor(u, dtype=torch.float32).to(self.device).contiguous() for u in (gate, draw)]
        check(self._e.set_scheduled_sampling(self._h, float(ss_prob), ptr(keep[0]), ptr(keep[1])))
        self._ss_live = keep           # the library reads them during the next xe_forward

    def xe_backward(self, grads, smoothing=0.1, n_tokens_global=0.0):
        """LabelSmoothingLoss + backward (Utils.py:268-286) for the last xe_forward(); returns the loss."""
        loss = torch.zeros(1, device=self.device)
        gs = self._grad_struct(grads)
        check(self._e.xe_backward(self._h, float(smoothing), C.byref(gs), ptr(loss), float(n_tokens_global), stream_ptr()))
        return loss

    def beam_search(self, feats, beam_size=5, max_steps=50):
        """The decoder's beam_search_sample (e.g. BUTD_Model.py:236-318) for all images of `feats` at once.
        Returns (seqs float32 (n_img, max_steps+1) zero-padded, lens int32 (n_img,)); row i[:lens[i]] is what the
        reference returns for image i (leading <sta>, trailing <end> if finished)."""
        feats = self._feats(feats)
        n = feats.shape[0]
        seqs = torch.zeros(n, max_steps + 1, dtype=torch.float32, device=feats.device)
        lens = torch.zeros(n, dtype=torch.int32, device=feats.device)
        check(self._e.beam_search(self._h, ptr(feats), n, beam_size, max_steps, ptr(seqs), ptr(lens), stream_ptr()))
        return seqs, lens

    def beam_search_opts(self, feats, beam_size=5, max_steps=50, n_best=1, length_penalty=None, block_ngram=0, groups=1, diversity=0.0):
        """beam_search with options (include/icz.h: icz_beam_opts): the n_best best of each image's beam_size hypotheses,
        ranked finished first, then by the length-penalised score (None | ('avg' | 'wu', alpha) | 'avg_<alpha>' | 'wu_<alpha>');
        block_ngram = n (2, 3, 4; 0 = off) forbids repeating an n-gram of the prefix.  Returns (seqs float32 (n_img, n_best,
        max_steps+1) zero-padded, lens int32 (n_img, n_best), raw log-prob scores (n_img, n_best)); the defaults give beam_search.
        groups > 1 (dividing beam_size) runs diverse beam search (icz_beam_diversity): the beam splits into `groups` groups, and
        each step a group's choice of a token is penalised by `diversity` for every earlier group that chose it at that step."""
        opts = _beam.make_opts(n_best, length_penalty, block_ngram)        # ValueError before the features are looked at
        div = _beam.make_diversity(groups, diversity, beam_size)
        return _beam.search(self._e, self._h, self._feats(feats), beam_size, max_steps, opts, div)

    def sample_decode(self, feats, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None):
        """Beyond the reference (include/icz.h: icz_*_sample_decode): n = 1..8 captions per image drawn in evaluation mode from
        softmax(logits / temperature) restricted to the top_k largest tokens (0 = off) and then to the nucleus of mass top_p
        (1 = off).  rng: None / an integer Philox seed, or explicit uniforms (max_len, B n) fp32 on the device.  Returns (ids int64
        (B n, max_len) with the drawn <end> and 0 behind it, the model's own log-prob of every token (B n, max_len), their sum
        (B n,)), row img * n + j.  Bad options raise ValueError before the features are looked at."""
        opts = _sampling.make_sample_opts(temperature, top_k, top_p, n)
        if top_k > self.V:
            raise ValueError("top_k %d above the vocabulary size %d" % (top_k, self.V))
        return _sampling.decode(self._e.sample_decode, self._h, self._feats(feats), int(n), int(max_len), opts, rng, self.max_rows)


class GraphDecoderHandle(DecoderHandle):
    """A family whose library handle takes options, captures hipGraphs and reports gradient groups: BUTD and AoA.  NIC has
    neither entry, and callers ask with hasattr()."""

    def enable_graphs(self, on):
        """Capture the SCST rollouts and the REINFORCE backward pass (BUTD: greedy / sample as well) into hipGraphs and replay
        them (include/icz.h: icz_*_set_option).  Implies persistent output buffers: the tensors those calls return are reused
        (overwritten) by the next call of the same shape."""
        self._persistent = bool(on)
        self.set_option("graphs", 1 if on else 0)

    def set_option(self, name, value):
        """icz_<family>_set_option (include/icz.h): "graphs", "early_out", ...; the family's header comment lists its own."""
        check(self._e.set_option(self._h, name.encode(), int(value)))
        self._option_set(name, int(value))

    def _option_set(self, name, value):
        """What an accepted option changes on the host side (AoA: "train_refiner" unfreezes the refiner's gradient buffers)."""

    def set_grad_callback(self, fn):
        """fn(stage) is called while a backward call is being enqueued, each time a group of gradients is complete in
        stream order (include/icz.h: icz_*_set_grad_callback); None removes it."""
        self._grad_cb = _lib.GRAD_READY_CB(lambda user, stage: fn(int(stage))) if fn is not None else _lib.GRAD_READY_CB()
        check(self._e.set_grad_callback(self._h, self._grad_cb, None))


class CaptionerBase(ScheduledSamplingState):
    """The Captioner methods of the reference (Models/*_Model.py) over a DecoderHandle, mixed in before nn.Module.  A subclass
    declares `_Handle`, builds its parameter tree, sets `dims` (the handle's leading constructor arguments) and defines
    `_features`; every forward / sampling / search path runs in the HIP library (no torch compute, no CPU fallback)."""

    _Handle = None

    def _decode_init(self, max_batch, max_beam, max_len):
        self.max_rows, self.max_len = max_batch * max(1, max_beam), max_len
        self._h = self._bound = self._rh = None
        self._seed = 0x5EED
        self._ss_init()                 # ss_prob (Engine.py:143) and its plumbing: scheduled.py

    def _named(self):
        sd = dict(self.decoder.named_parameters())
        return {k: sd[k] for k in self._Handle._param_keys}

    def _new_handle(self, max_rows, max_len, device):
        return self._Handle(*self.dims, max_rows, max_len, device)

    def _features(self, visual_inputs):
        """What the samplers hand the handle for `visual_inputs`."""
        raise NotImplementedError

    def _handle(self):
        """(Re)bind the handle when parameters moved (.to(device), load_state_dict keeps storage) and refresh the
        materialised weight-norm weights -- cheap (4 small kernels) and always correct after optimizer steps."""
        named = self._named()
        ptrs = tuple(p.data_ptr() for p in named.values())
        dev = next(iter(named.values())).device
        if dev.type != "cuda":
            raise RuntimeError("%s (libicz) needs its parameters on a ROCm device; got %s" % (type(self).__name__, dev))
        fresh = self._h is None or self._h.device != dev
        if fresh:
            self._h = self._new_handle(self.max_rows, max(self.max_len, 20), dev)
            self._bound = None
        if ptrs != self._bound:
            self._h.bind({k: p.data for k, p in named.items()})
            self._bound = ptrs
        else:
            self._h.refresh()
        self._ss_push(self._h, fresh)
        self._push_options(self._h)
        return self._h

    def _push_options(self, h):
        """Captioner attributes that are handle options (AoA: train_refiner); called by _handle()."""

    def _replay_handle(self):
        """One-row handle for the teacher-forced replay behind eval_test_image's attention maps: the training handle keeps its
        stored forward pass, its captured graphs and its buffers (a beam sentence of up to 50 steps would re-allocate them),
        and the replay never sees scheduled sampling (a fresh handle has it switched off)."""
        named = self._named()
        dev = next(iter(named.values())).device
        if self._rh is None or self._rh.device != dev:
            self._rh = self._new_handle(1, 52, dev)
        self._rh.bind({k: p.data for k, p in named.items()})       # binds and refreshes: the parameters may have moved on
        return self._rh

    def _next_rng(self):
        from .dist import seed_for_rank
        self._seed += 1
        return self._Handle._make_rng(seed_for_rank(self._seed))       # data-parallel replicas draw independent streams

    def get_param_groups(self, lr_dict):
        """Only the decoder is optimised (BUTD_Model.py:451-456, AoA_Model.py:669-674)."""
        return [{"params": list(self.decoder.parameters()), "lr": lr_dict["lr"]}]

    # ---- the methods Engine calls -------------------------------------------------------------------
    def forward(self, visual_inputs, captions, lengths, rng=None):
        """XE forward: [0] of the result = packed logits (sum(lengths), V) (fused path, no autograd graph: gradients come from
        the handle's xe_backward)."""
        train = self.training
        logits = self._handle().xe_forward(self._features(visual_inputs), captions, list(lengths),
                                           (rng or self._next_rng()) if train else None, train=train, want_logits=True)
        return (logits, None)

    def sampler(self, visual_inputs, max_len=20):
        """Greedy decode -> LongTensor (B, max_len)."""
        return self._handle().greedy(self._features(visual_inputs), max_len)

    def sampler_rl(self, visual_inputs, max_len=20, rng=None):
        """Multinomial rollout -> (seq LongTensor (B,T), seqLogprobs (B,T)) (fused path: use the handle's sample_backward)."""
        return self._handle().sample(self._features(visual_inputs), max_len, rng or self._next_rng())

    def sample_decode(self, visual_inputs, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None):
        """n sampled captions per image in evaluation mode with temperature / top-k / nucleus filtering (an extension; the handle's
        sample_decode) -> (ids (B n, max_len), log-probs (B n, max_len), scores (B n,)), row img * n + j."""
        return self._handle().sample_decode(self._features(visual_inputs), n, max_len, temperature, top_k, top_p, rng)

    def beam_search_sampler(self, visual_inputs, beam_size=5):
        """Beam search.  A batch of one image returns the reference's (1, L) float tensor; larger batches (an extension)
        return a list of (1, L_i) tensors."""
        seqs, lens = self._handle().beam_search(self._features(visual_inputs), beam_size, 50)
        lens = lens.tolist()
        out = [seqs[i:i + 1, :lens[i]] for i in range(len(lens))]
        return out[0] if len(out) == 1 else out

    def beam_search_nbest(self, visual_inputs, beam_size=5, n_best=None, length_penalty=None, block_ngram=0, groups=1, diversity=0.0):
        """Beam search returning each image's n-best list (an extension; include/icz.h: icz_beam_opts): per image a list of
        (ids float32 (1, L_i) with <sta> and, if finished, <end>; raw summed log-prob), best first; n_best=None = all beam_size
        hypotheses.  length_penalty (None, ('avg' | 'wu', alpha), 'avg_<alpha>', 'wu_<alpha>') ranks them; block_ngram = n
        forbids repeating an n-gram; groups > 1 with a diversity penalty runs diverse beam search (icz_beam_diversity)."""
        seqs, lens, scores = self._handle().beam_search_opts(self._features(visual_inputs), beam_size, 50, beam_size if n_best is None else n_best,
                                                             length_penalty, block_ngram, groups, diversity)
        return nbest_lists(seqs, lens, scores)

    @staticmethod
    def _words(ids, caption_vocab, stop_at_pad=False):
        """The words of one decoded row (a tensor or an array of ids) up to <end>, without <sta>: the tail of every eval_test_image
        and of the engine's caption lists.  stop_at_pad: the row also ends at its first <pad> (0), as a sampled row does."""
        caption, ix2word = [], caption_vocab.ix2word
        for word_id in (ids.cpu().numpy() if torch.is_tensor(ids) else ids):
            word = ix2word[int(word_id)]
            if word == "<end>" or (stop_at_pad and int(word_id) == 0):
                break
            elif word != "<sta>":
                caption.append(word)
        return caption
