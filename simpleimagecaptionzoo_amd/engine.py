"""Engine subclasses for the hot path (drop-ins for ModelEngines/BUTD_Engine.py on top of Engine.py).

Mirrors the reference's Engine methods that sit on the path -- same names, argument meaning, batch-tuple layouts
and output contract:
    modify_visual_inputs          BUTD_Engine.py:23-47
    training_epoch                Engine.py:169-188      (XE: forward, label-smoothed loss, backward, clamp 0.1, Adam)
    SCST_training_epoch           Engine.py:251-272      (greedy baseline, sampled rollout, CIDEr-D reward, REINFORCE,
                                                          clamp 0.25, Adam)
    eval_captions_json_generation Engine.py:274-300      (greedy or beam decode -> [{'image_id', 'caption'}])
Everything between the batch tuple and the updated parameters runs in libicz; the host only moves the feature batch
to the device and (for evaluation) turns ids into words.  With torch.distributed initialised (dist.py) the same
methods run data-parallel: per-rank shards, all-reduced loss normaliser and gradients.
"""
import json

import numpy as np
import torch

from ._lib import BUTD_PARAM_KEYS, check, lib, ptr, stream_ptr
from .beam import make_diversity, parse_length_penalty
from .sampling import make_sample_opts
from .multisample import sample_n
from .scst_objective import sample_backward_objective
from .captioner import BUTDDetection_Captioner
from .handle import CaptionerBase
from .ciderd import CiderDReward
from . import dist as icz_dist
from .features import wait_event


class FusedAdam:
    """clip_gradient (Utils.py:241-250) + torch.optim.Adam(betas=(0.9,0.999), eps=1e-8, weight_decay=0)
    (Utils.py:219-220) as one HIP kernel per parameter tensor.  Exposes param_groups like a torch optimizer so the
    reference's set_lr / get_lr helpers (Utils.py:231-239) keep working."""

    def __init__(self, params, lr):
        if isinstance(params, (list, tuple)) and params and isinstance(params[0], dict):
            self.param_groups = [dict(g) for g in params]
            for g in self.param_groups:
                g.setdefault("lr", lr)
        else:
            self.param_groups = [{"params": list(params), "lr": lr}]
        self.state = {}

    def zero_grad(self):
        pass

    def state_dict(self):
        """Same layout as torch.optim.Adam.state_dict(): parameters are numbered in param_groups order.  (The reference
        neither saves the optimizer, Engine.py:81-88, nor keeps it across epochs, Engine.py:133-136; with this a caller
        can -- SURVEY.md 8f row 4.)"""
        index, groups = {}, []
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                index.setdefault(p, len(index))
                ids.append(index[p])
            groups.append({**{k: v for k, v in g.items() if k != "params"}, "betas": (0.9, 0.999), "eps": 1e-8,
                           "weight_decay": 0, "params": ids})
        state = {index[p]: {"step": torch.tensor(float(st["step"])), "exp_avg": st["exp_avg"].clone(),
                            "exp_avg_sq": st["exp_avg_sq"].clone()} for p, st in self.state.items()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        params = [p for g in self.param_groups for p in g["params"]]
        have, want = [len(g["params"]) for g in sd["param_groups"]], [len(g["params"]) for g in self.param_groups]
        if have != want:
            raise ValueError("optimizer state has a different parameter grouping: the checkpoint holds %s parameters per group, this optimizer "
                             "%s (an AoA checkpoint written without train_refiner does not load into an optimizer made with it, or the "
                             "reverse: create the optimizer from the same get_param_groups)" % (have, want))
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g["lr"] = saved["lr"]
        self.state = {}
        for i, st in sd["state"].items():
            p = params[int(i)]
            self.state[p] = {"step": int(float(st["step"])), "exp_avg": st["exp_avg"].to(p.device, torch.float32).clone(),
                             "exp_avg_sq": st["exp_avg_sq"].to(p.device, torch.float32).clone()}

    def step_with(self, grads_by_param, clip):
        """grads_by_param: {parameter: gradient tensor}.  One multi-tensor launch per param group."""
        import ctypes as C
        for group in self.param_groups:
            ps = [p for p in group["params"] if grads_by_param.get(p) is not None]
            if not ps:
                continue
            steps = set()
            for p in ps:
                st = self.state.get(p)
                if st is None:
                    st = {"step": 0, "exp_avg": torch.zeros_like(p.data), "exp_avg_sq": torch.zeros_like(p.data)}
                    self.state[p] = st
                st["step"] += 1
                steps.add(st["step"])
            assert len(steps) == 1, "parameters of one group share the step count"
            n = len(ps)
            for lo in range(0, n, 32):
                chunk = ps[lo:lo + 32]
                m = len(chunk)
                arr = lambda xs: (C.c_void_p * m)(*xs)
                check(lib().icz_adam_clamp_multi(
                    m, arr([p.data.data_ptr() for p in chunk]), arr([grads_by_param[p].data_ptr() for p in chunk]),
                    arr([self.state[p]["exp_avg"].data_ptr() for p in chunk]),
                    arr([self.state[p]["exp_avg_sq"].data_ptr() for p in chunk]),
                    (C.c_int64 * m)(*[p.numel() for p in chunk]), float(group["lr"]), float(clip), steps.pop() if lo + 32 >= n else next(iter(steps)),
                    stream_ptr()))


def init_optimizer(optimizer_type, params, learning_rate):
    """Utils.py:222-229 (Adam only on the fused path)."""
    if optimizer_type != "Adam":
        raise ValueError("the fused optimiser implements Adam (the reference's default, Main.py:171)")
    if len(params) == 0:
        return None
    return FusedAdam(params, learning_rate)


class Engine(object):
    """The part of Engine.py:16-41 the hot path needs (construction, device, vocabulary, tag)."""

    def __init__(self, model_settings_json, dataset_name, caption_vocab, data_dir=None, use_bu="unused", device="cuda:0",
                 cider_df=None, max_batch=128):
        if isinstance(model_settings_json, dict):
            self.settings = dict(model_settings_json)
        else:
            self.settings = json.load(open(model_settings_json, "r"))
        self.device = torch.device(device)
        self.data_dir = data_dir
        self.dataset_name = dataset_name
        self.use_bu = use_bu
        self.caption_vocab = caption_vocab
        self.tag = "Model_" + self.settings["model_type"] + "_Dataset_" + dataset_name
        self.model = self.model_construction(max_batch)
        self.model.to(self.device)
        self.cnn_ft_model = 0
        self._cider_df = cider_df
        self._scorer = None
        self._pinned = None
        self._dev_feats = None
        self.use_graphs = True      # replay captured hipGraphs in SCST / greedy evaluation (buffers are persistent)
        # data-parallel: start each gradient group's all-reduce from the library's gradient-ready callback, beside the rest of the backward
        # pass (default); False (or ICZ_DP_OVERLAP=0) = ONE all-reduce of the flat buffer behind the backward pass -- the A/B leg
        # bench.py reports as `dp_overlap`
        import os
        self.dp_overlap = os.environ.get("ICZ_DP_OVERLAP", "1") not in ("0", "")
        self.phase_events = None    # a list: every SCST step appends its phase-boundary events (phase_times() turns them into ms)
        self.scst_terms = None      # a list: every SCST step run with an objective appends its (obj, ent) pair of 1-element device tensors
        # The hot path runs on its own non-default stream: after hipGraph replays, eager launches on the legacy null
        # stream were measured 2-3x slower on ROCm 7.2 (implicit synchronisation with the graph's internal streams).
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def model_construction(self, max_batch):
        raise NotImplementedError

    # ---- checkpoints: the reference's files (Engine.py:43-70, 81-88) + the optimizer state next to them
    def _cp_paths(self, scst, root=None):
        import os
        flag = "scst_" if scst else ""
        cp_dir = os.path.join(root or "./CheckPoints/%s/" % self.tag, "cp")
        return cp_dir, os.path.join(cp_dir, "Captioner_%scp.pth" % flag), os.path.join(cp_dir, "%sstate_histories.json" % flag), \
            os.path.join(cp_dir, "Optimizer_%scp.pth" % flag)

    def save_checkpoint(self, cider_scores, save_scst_model=False, optimizer=None, root=None):
        """Engine.py:81-88: model state_dict + score history, same file names; with `optimizer` also its state
        (`Optimizer_[scst_]cp.pth`, torch.optim layout) -- the reference re-creates Adam every epoch (Engine.py:133-136) and
        loses the moments at every restart."""
        import os
        cp_dir, model_path, his_path, opt_path = self._cp_paths(save_scst_model, root)
        os.makedirs(cp_dir, exist_ok=True)
        torch.save(self.model.state_dict(), model_path)
        json.dump({"cider_his": cider_scores}, open(his_path, "w"))
        if optimizer is not None:
            torch.save(optimizer.state_dict(), opt_path)

    def load_from_checkpoint(self, load_scst_model=False, load_best=False, optimizer=None, root=None):
        """Engine.py:43-70 (same files, same return value) + the optimizer state when `optimizer` is given and the file exists."""
        import os
        cp_dir, model_path, his_path, opt_path = self._cp_paths(load_scst_model, root)
        cider_his, start_epoch = [], 1
        best_not_found = False
        if load_best:
            best = os.path.join(os.path.dirname(cp_dir), "best", os.path.basename(model_path))
            if os.path.exists(best):
                self.model.load_state_dict(torch.load(best, map_location=self.device))
            else:
                best_not_found = True
        if not load_best or best_not_found:
            if os.path.exists(his_path):
                cider_his = json.load(open(his_path, "r"))["cider_his"]
            if os.path.exists(model_path):
                self.model.load_state_dict(torch.load(model_path, map_location=self.device))
            else:
                print("recent checkpoint not found.")
            if optimizer is not None and os.path.exists(opt_path):
                optimizer.load_state_dict(torch.load(opt_path, map_location=self.device))
            start_epoch = len(cider_his) + 1
        return cider_his, start_epoch

    def SCST_multisample_training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5):
        """Beyond the reference, for every decoder family (BUTD, AoA -- also with train_refiner -- and NIC): the multi-sample SCST
        step.  K = samples_per_image (2..8) captions are sampled per image (multisample.sample_n: the per-image work runs once per
        image), each is baselined by the mean CIDEr-D of the image's other K - 1 (reward_loo), and there is no greedy rollout; the
        mask-sum exchange, the gradient-reduce hooks, the 0.25 clamp and Adam are SCST_training_epoch's.  B K must fit the handle's
        row capacity.  ValueError for a K outside 2..8, a bool or a non-integer, before any device work.  (Other objectives over the
        same K samples: SCST_objective_training_epoch.)"""
        from .multisample import check_samples
        k = check_samples(samples_per_image)
        with _on_stream(self):
            return self._scst_training_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs, k)

    def SCST_objective_training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5,
                                      objective="loo", risk_alpha=1.0, entropy_weight=0.0):
        """SCST_multisample_training_epoch (same arguments in front, every decoder family) with the objective to choose (beyond the
        reference; scst_objective.py): objective "loo" is that method's leave-one-out reward through RewardCriterion, "risk" is
        minimum-risk training over the K samples of an image with sharpness risk_alpha (finite, > 0); entropy_weight > 0 (finite)
        subtracts that multiple of the mean per-step entropy of the word distribution from the loss.  The defaults run
        SCST_multisample_training_epoch's calls exactly.  The returned list stays the total loss per step; while `scst_terms` is a
        list every step run with an objective appends its (obj, ent) device pair.  Data-parallel, "risk" divides by the all-reduced
        image count.  ValueError for a bad samples_per_image, objective, risk_alpha or entropy_weight before any device work."""
        from .multisample import check_samples
        k = check_samples(samples_per_image)
        if objective not in ("loo", "risk"):
            raise ValueError("objective must be 'loo' or 'risk', got %r" % (objective,))
        obj = _scst_objective_args(objective == "risk", k, risk_alpha, entropy_weight)
        with _on_stream(self):
            return self._scst_training_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs, k, obj)

    def SCST_distinct_training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5,
                                     estimator="normalised"):
        """Beyond the reference, for every decoder family: SCST on samples drawn WITHOUT replacement (swor.py).  Per step,
        n = samples_per_image (3..8) distinct captions per image come from stochastic beam search at temperature 1 in evaluation
        mode (stochastic_beam.sample_distinct); the last slot of an image is only the threshold, its n - 1 others are the samples;
        every slot is scored by CIDEr-D; the samples go through a training-mode teacher-forced forward (dropout on) and
        xe_backward_swor weighs them: estimator "normalised" (default; biased, low variance) or "unbiased".  The gradient-reduce
        hooks, the 0.25 clamp and Adam are SCST_training_epoch's; data-parallel, the all-reduced image count is the normaliser.
        `rngs` (tests) supplies per batch a pair (sample_distinct's rng, the forward's icz_rng).  Returns the loss per step; the
        per-step stats (images, 3) = {W, baseline, effective sample size} stay in self.last_swor_stats.  Every row of the forward
        repeats its image's features and per-image prologue.  ValueError, before any device work, for a bad samples_per_image or
        estimator, B n above the handle's row capacity, scheduled sampling live, or a batch with per-image region counts
        (repeating a RegionBatch per row is out of this method's scope)."""
        from .swor import check_args
        n, _, _ = check_args(samples_per_image, estimator)
        if self.model.scheduled_sampling and float(self.model.ss_prob) > 0.0:
            raise ValueError("scheduled sampling is live (ss_prob %g): the forward pass would be fed other tokens than the sampled captions"
                             % float(self.model.ss_prob))
        with _on_stream(self):
            return self._scst_distinct_training_epoch(dataloader, optimizer, tqdm_visible, rngs, n, estimator)


def _check_distinct_batch(n_img, n, max_rows, supp_info_datas):
    """The per-batch refusals of SCST_distinct_training_epoch, looked at before the step touches the device"""
    if n_img * n > max_rows:
        raise ValueError("%d images x %d slots exceed the handle's row capacity %d" % (n_img, n, max_rows))
    if _has_region_counts(supp_info_datas):
        raise ValueError("a batch with per-image region counts: SCST on distinct samples repeats one feature tensor per row")


def _has_region_counts(supp_info_datas):
    """whether a batch carries per-image region counts (a resident batch with `bu_counts`, or host features of unequal row counts)"""
    if isinstance(supp_info_datas, dict):
        return supp_info_datas.get("bu_counts") is not None
    try:
        return len({int(s["bu_feat"].shape[0]) for s in supp_info_datas}) > 1
    except (TypeError, KeyError, IndexError, AttributeError):
        return False


def _scst_objective_args(risk, k, risk_alpha, entropy_weight):
    """The objective arguments of an SCST epoch (risk: minimum-risk training, else the step's reward) -> None (today's calls: the
    reward through RewardCriterion, no entropy term) or the scst_objective.Objective every step attaches its reward / scores to;
    ValueError for a bad argument."""
    from .scst_objective import make_objective
    obj = make_objective("risk" if risk else "reinforce", k, risk_alpha, entropy_weight)
    return None if not risk and obj.entropy_weight == 0.0 else obj


class BUTDDetection_Eng(Engine):
    """ModelEngines/BUTD_Engine.py:21-47 + the three hot Engine methods on libicz.
    `use_bu='adaptive'` (10..100 boxes per image, Main.py:158; beyond the reference, whose BUTD model drops the mask this engine
    builds): the handle is sized for `num_regions` (default 100) and every batch carries its region counts."""

    def model_construction(self, max_batch):
        s = self.settings
        assert s["model_type"] in ("BUTDDetection", "BUTDSpatial")
        model = BUTDDetection_Captioner(atten_dim=s["atten_dim"], embed_dim=s["embed_dim"], hidden_dim=s["hidden_dim"],
                                        vocab_size=len(self.caption_vocab), device=str(self.device),
                                        num_regions=s.get("num_regions", 100 if self.use_bu == "adaptive" else 36), enc_dim=s.get("enc_dim", 2048),
                                        max_batch=max_batch)
        model.region_masks = self.use_bu == "adaptive"
        return model

    # ---- E4 -------------------------------------------------------------------------------------------------
    def modify_visual_inputs(self, img_tensors, supp_info_datas=None):
        """BUTD_Engine.py:23-47: stack per-image (n_i, D) features into (B, max_n, D) fp32 + mask (None if all
        rows are full).  Staged through a reusable pinned buffer and copied asynchronously."""
        if isinstance(supp_info_datas, dict) and torch.is_tensor(supp_info_datas.get("bu_feats")):
            # extension: a batch already resident in HBM (prefetching loaders, bench.py); padded batches carry their counts
            feats, counts = supp_info_datas["bu_feats"], supp_info_datas.get("bu_counts")
            if self.use_graphs and counts is None and feats.is_cuda:
                # captured graphs are keyed by the feature tensor's address: a prefetching loader's ring of `depth` buffers replays
                # them, any other tensor is copied (device to device, ~7 us for 19 MB) into ONE persistent buffer first.  The
                # address set belongs to one loader instance: a new one (e.g. per epoch) starts it afresh
                ring = supp_info_datas.get("bu_ring")
                token, depth = ring if isinstance(ring, tuple) else (None, 0)
                cache = self.__dict__.setdefault("_feat_ring", {"token": None, "addrs": set()})
                if token is not None and cache["token"] != token:
                    cache["token"], cache["addrs"] = token, set()
                seen = cache["addrs"] if token is not None else ()
                if feats.data_ptr() not in seen:
                    if token is not None and len(seen) < depth:
                        seen.add(feats.data_ptr())
                    else:
                        buf = getattr(self, "_dev_batch", None)
                        if buf is None or buf.shape != feats.shape:
                            buf = self._dev_batch = torch.empty_like(feats, memory_format=torch.contiguous_format)
                        buf.copy_(feats, non_blocking=True)
                        feats = buf
            out = {"bu_feats": feats, "bu_bboxes": supp_info_datas.get("bu_bboxes"), "bu_masks": None}
            if counts is not None:
                out["bu_masks"] = (torch.arange(feats.shape[1]).unsqueeze(0) < torch.tensor(counts).unsqueeze(1)).float().to(self.device)
                out["bu_counts"] = list(counts)
            return out
        bu_feats = [s["bu_feat"] for s in supp_info_datas]
        bu_bboxes = [s["bu_bbox"] for s in supp_info_datas]
        counts = [int(f.shape[0]) for f in bu_feats]
        max_len = max(counts)
        B, D = len(bu_feats), bu_feats[0].shape[1]
        # flat staging buffers sized for the largest batch seen: 'adaptive' batches change max_len every step
        need = B * max_len * D
        if self._pinned is None or self._pinned.numel() < need:
            self._pinned = torch.zeros(need, dtype=torch.float32).pin_memory()
            self._dev_feats = torch.empty(need, dtype=torch.float32, device=self.device)
        if getattr(self, "_h2d_done", None) is not None:
            wait_event(self._h2d_done)           # the previous batch's copy has left the pinned buffer
        host = self._pinned[:need].view(B, max_len, D)
        hv = host.numpy()
        for i, f in enumerate(bu_feats):
            hv[i, :counts[i]] = f
            if counts[i] < max_len:
                hv[i, counts[i]:] = 0
        # a persistent device buffer: a stable address lets the captured graphs be replayed
        feats = self._dev_feats[:need].view(B, max_len, D)
        feats.copy_(host, non_blocking=True)
        self._h2d_done = torch.cuda.Event()
        self._h2d_done.record()
        if min(counts) == max_len:
            return {"bu_feats": feats, "bu_bboxes": bu_bboxes, "bu_masks": None}
        masks = (torch.arange(max_len).unsqueeze(0) < torch.tensor(counts).unsqueeze(1)).float().to(self.device)
        # `bu_counts` (extension): the counts behind the prefix mask, so that the Captioner need not read the mask back
        return {"bu_feats": feats, "bu_bboxes": bu_bboxes, "bu_masks": masks, "bu_counts": counts}

    # ---- helpers ------------------------------------------------------------------------------------------
    # Gradient groups in the order the backward pass completes them (include/icz.h: icz_butd_set_grad_callback); the flat
    # buffer is laid out group by group so that each group is one contiguous slice = one all-reduce.
    _GRAD_STAGES = (("predict.weight_v", "predict.weight_g", "predict.bias"),
                    ("embed.0.weight", "TD_atten.weight_ih", "TD_atten.weight_hh"),
                    ("language_model.weight_ih", "language_model.weight_hh"))

    def _grads(self):
        """Gradient buffers as views into ONE flat fp32 buffer (few large all-reduces over xGMI move them all)."""
        if getattr(self, "_flat", None) is None:
            named = self._trainable()
            staged = [k for st in self._GRAD_STAGES for k in st if k in named]
            order = staged + [k for k in named if k not in staged]
            offs, total, bounds = {}, 0, []
            for k in order:
                offs[k] = total
                total += (named[k].numel() + 63) // 64 * 64
                bounds.append(total)
            self._flat = torch.zeros(total, dtype=torch.float32, device=self.device)
            self._gviews = {k: self._flat[offs[k]:offs[k] + named[k].numel()].view_as(named[k]) for k in named}
            # slice of the flat buffer per stage (+ the remainder), only meaningful when every staged key is present
            self._stage_slices = []
            if len(staged) == sum(len(st) for st in self._GRAD_STAGES):
                lo, i = 0, 0
                for st in self._GRAD_STAGES:
                    i += len(st)
                    self._stage_slices.append((lo, bounds[i - 1]))
                    lo = bounds[i - 1]
                self._stage_slices.append((lo, total))
        return self._gviews

    def _reduce_grads_begin(self, h):
        """Data-parallel: start the all-reduce of each gradient group as soon as the backward pass has enqueued it, so that
        RCCL moves it over xGMI beside the remaining weight-gradient GEMMs (the hook is a no-op for one process)."""
        self._pending = []
        if not icz_dist.is_distributed() or not self._stage_slices or not hasattr(h, "set_grad_callback"):
            return False
        if not self.dp_overlap:
            if getattr(self, "_hooked", None) is h:
                h.set_grad_callback(None)
                self._hooked = None
            return False
        if getattr(self, "_hooked", None) is not h:
            import torch.distributed as td

            def on_ready(stage):
                try:      # called from inside the C library: an exception cannot propagate through it
                    lo, hi = self._stage_slices[stage]
                    self._pending.append(td.all_reduce(self._flat[lo:hi], op=td.ReduceOp.SUM, async_op=True))
                except Exception as e:      # re-raised by _reduce_grads_end
                    self._hook_error = e
            h.set_grad_callback(on_ready)
            self._hooked = h
        return True

    def _reduce_grads_end(self, overlapped):
        if not icz_dist.is_distributed():
            return
        if not overlapped:
            icz_dist.all_reduce_sum_(self._flat)
            return
        err, self._hook_error = getattr(self, "_hook_error", None), None
        if err is not None or len(self._pending) != len(self._stage_slices) - 1:
            raise RuntimeError("gradient hook: %d of %d groups were reduced%s" % (
                len(self._pending), len(self._stage_slices) - 1, "" if err is None else " (%r)" % (err,)))
        lo, hi = self._stage_slices[-1]
        icz_dist.all_reduce_sum_(self._flat[lo:hi])
        for w in self._pending:
            w.wait()
        self._pending = []

    def _features(self, visual_inputs):
        """What the decoder handle consumes: the captioner's own hook (bottom-up features, AoA: with the region counts, NIC: the
        image embedding)."""
        return self.model._features(visual_inputs)

    def _trainable(self):
        """name -> parameter for everything the optimizer updates (AoA: the decoder only, AoA_Model.py:669-674)."""
        return getattr(self.model, "_trainable", self.model._named)()

    def _apply(self, optimizer, clip):
        named = self._trainable()
        grads = self._gviews
        if isinstance(optimizer, FusedAdam):
            optimizer.step_with({named[k]: grads[k] for k in grads}, clip)
        else:   # a torch optimizer handed in by unmodified reference code
            for k in grads:
                named[k].grad = grads[k].clamp(-clip, clip)
            optimizer.step()

    def scorer(self):
        if self._scorer is None:
            df = self._cider_df
            if df is None:
                raise RuntimeError("SCST needs the CIDEr document-frequency table: pass cider_df={'document_frequency':"
                                   " ..., 'ref_len': n} (the content of cider/data/<dataset>-train.p)")
            if isinstance(df, str):
                import pickle
                df = pickle.load(open(df, "rb"), encoding="latin1")
            self._scorer = CiderDReward(df["document_frequency"], df["ref_len"], self.caption_vocab.word2ix, self.device)
            self._scorer.persistent = True
        return self._scorer

    def _hot_handle(self):
        h = self.model._handle()
        if self.use_graphs != h._persistent:
            h.enable_graphs(self.use_graphs)
        return h

    # ---- E1 -------------------------------------------------------------------------------------------------
    def training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None):
        with _on_stream(self):
            return self._training_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs)

    def _xe_token_norm(self, h, lengths):
        """The `n_tokens_global` of an XE backward call: 0 (the local count) for one process.  Data-parallel, G2: every
        rank scales by 1 / (global token count); the count is all-reduced on the device and handed to the library as a device scalar
        (-1: no host round trip between forward and backward)."""
        if not icz_dist.is_distributed():
            return 0.0
        n_dev = torch.full((1,), float(sum(lengths)), dtype=torch.float32, device=self.device)
        if hasattr(h, "set_mask_sum_global"):
            icz_dist.all_reduce_sum_(n_dev)
            h.set_mask_sum_global(n_dev)
            return -1.0
        return icz_dist.all_reduce_scalar(n_dev)

    def _training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None):
        """Engine.py:169-188.  `criterion` is the reference's LabelSmoothingLoss (only its .smoothing is read: the
        loss and its gradient are fused into the backward kernels).  `rngs` (tests) supplies one icz_rng per batch."""
        return self._xe_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs, "Training Process",
                              lambda *batch: lambda h, grads, smoothing, n_glob: h.xe_backward(grads, smoothing, n_glob))

    def _xe_epoch(self, dataloader, optimizer, criterion, tqdm_visible, rngs, desc, begin):
        """The XE epoch of _training_epoch and _distill_training_epoch.  What varies is the backward call: begin(img_tensors,
        supp_info_datas, captions, lengths) runs in front of the student's forward pass and returns backward(h, grads, smoothing,
        n_glob) -> loss."""
        self.model.train()
        smoothing = float(getattr(criterion, "smoothing", 0.0))
        monitor = _monitor(dataloader, desc, tqdm_visible)
        losses = []
        for batch_i, (img_ids, img_tensors, captions, lengths, supp_info_datas) in enumerate(monitor):
            visual_inputs = self.modify_visual_inputs(img_tensors, supp_info_datas)
            lengths = [cap_len - 1 for cap_len in lengths]
            backward = begin(img_tensors, supp_info_datas, captions, lengths)
            h = self.model._handle()
            rng = rngs[batch_i] if rngs is not None else self.model._next_rng()
            h.xe_forward(self._features(visual_inputs), captions, lengths, rng, train=True)
            grads = self._grads()
            n_glob = self._xe_token_norm(h, lengths)
            ov = self._reduce_grads_begin(h)
            loss = backward(h, grads, smoothing, n_glob)
            self._reduce_grads_end(ov)
            self._apply(optimizer, 0.1)
            losses.append(loss)
            if tqdm_visible:
                monitor.set_postfix(Loss=np.round(loss.item(), decimals=4))
        return losses

    # decoders with a grouped XE forward (icz_butd_xe_forward_n); the AoA and NIC engines refuse training_epoch_grouped
    _grouped_xe = True

    def training_epoch_grouped(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, captions_per_image=5):
        """Beyond the reference: the XE epoch on K = captions_per_image (2..8) references per image, the regime of seq_per_img = 5.
        `dataloader` is the SCST loader: batches (img_ids, img_tensors, img_gts, supp_info_datas).  Per step the features of the B
        images are staged once, grouped.make_batch encodes the first K references of every image into image-major rows, and
        grouped.xe_forward_n runs the per-image work once per image and the decoder chain over the B K rows; the token-count
        exchange, the gradient-reduce hooks, xe_backward with criterion.smoothing, the 0.1 clamp and Adam are training_epoch's.
        Per-image region counts are honoured.  BUTD decoders: BUTDDetection_Eng and BUTDSpatial_Eng (the same decoder over the 49
        grid regions) run it; AoADetection_Eng and NIC_Eng raise NotImplementedError (their grouped forward is the follow-up).
        ValueError, before any device work, for a bad captions_per_image, scheduled sampling live, an image with fewer than K
        references, or a batch whose B K exceeds the handle's row capacity."""
        from .grouped import check_captions_per_image
        if not self._grouped_xe:
            raise NotImplementedError("%s has no grouped XE forward yet: icz_butd_xe_forward_n serves the BUTD decoders; the AoA and NIC "
                                      "forms (icz_aoa_xe_forward_n, icz_nic_xe_forward_n) are the follow-up" % type(self).__name__)
        k = check_captions_per_image(captions_per_image)
        if self.model.scheduled_sampling and float(self.model.ss_prob) > 0.0:
            raise ValueError("scheduled sampling is live (ss_prob %g): the grouped forward feeds the captions' own tokens" % float(self.model.ss_prob))
        with _on_stream(self):
            return self._training_epoch_grouped(dataloader, optimizer, criterion, tqdm_visible, rngs, k)

    def _training_epoch_grouped(self, dataloader, optimizer, criterion, tqdm_visible, rngs, k):
        """training_epoch_grouped's steps: those of _xe_epoch with make_batch and xe_forward_n in the place of the loader's rows"""
        from .grouped import make_batch, xe_forward_n
        self.model.train()
        smoothing = float(getattr(criterion, "smoothing", 0.0))
        monitor = _monitor(dataloader, "Training Process", tqdm_visible)
        losses = []
        for batch_i, (img_ids, img_tensors, img_gts, supp_info_datas) in enumerate(monitor):
            if len(img_ids) * k > self.model.max_rows:      # before the step's device work
                raise ValueError("%d images x %d captions exceed the handle's row capacity %d" % (len(img_ids), k, self.model.max_rows))
            captions, lengths = make_batch(self.caption_vocab, img_ids, img_gts, k)
            visual_inputs = self.modify_visual_inputs(img_tensors, supp_info_datas)
            lengths = [cap_len - 1 for cap_len in lengths]
            h = self.model._handle()
            rng = rngs[batch_i] if rngs is not None else self.model._next_rng()
            xe_forward_n(h, self._features(visual_inputs), captions, lengths, k, rng, train=True)
            grads = self._grads()
            n_glob = self._xe_token_norm(h, lengths)
            ov = self._reduce_grads_begin(h)
            loss = h.xe_backward(grads, smoothing, n_glob)
            self._reduce_grads_end(ov)
            self._apply(optimizer, 0.1)
            losses.append(loss)
            if tqdm_visible:
                monitor.set_postfix(Loss=np.round(loss.item(), decimals=4))
        return losses

    def distill_training_epoch(self, dataloader, optimizer, criterion, teachers, tqdm_visible=True, rngs=None, *, alpha=0.5, temperature=1.0,
                               weights=None):
        """Beyond the reference: training_epoch with the word-level distillation loss of distill.py in the place of the XE loss.
        `teachers` = 1..4 other Engines of the same vocabulary on the same device, any mix of families, in evaluation mode for
        the epoch; every step each turns the shared batch into its own features (its modify_visual_inputs and _features, as
        eval_ensemble_captions_json_generation does) and runs a teacher-forced forward on the batch's captions, and the student's
        backward pass starts from loss = ((1 - alpha) hard + alpha temperature^2 KL(q || softmax(s / temperature))) / N with q the
        `weights`-averaged (None = uniform) teacher distribution at `temperature`.  The token-count exchange, the gradient-reduce
        hooks, the 0.1 clamp, Adam and criterion.smoothing are training_epoch's.  Returns the losses; the per-step (hard, kd) terms
        stay in self.last_distill_terms.  ValueError, before any device work, for 0 or more than 4 teachers, this engine among
        them, a vocabulary or device mismatch, a bad alpha, temperature or weights, or scheduled sampling live on the student (the
        teachers would be fed other tokens than the student)."""
        from .distill import check_opts
        teachers = list(teachers)
        check_opts(len(teachers), weights, alpha, temperature, float(getattr(criterion, "smoothing", 0.0)))
        if any(t is self or t.model is self.model for t in teachers):
            raise ValueError("the student is among its teachers: a teacher's forward pass would replace the student's stored one")
        if len({len(e.caption_vocab) for e in teachers + [self]}) != 1:
            raise ValueError("the vocabularies differ in size: student %d, teachers %s" % (len(self.caption_vocab), [len(e.caption_vocab) for e in teachers]))
        if len({str(e.device) for e in teachers + [self]}) != 1:
            raise ValueError("the engines sit on different devices %s" % [str(e.device) for e in [self] + teachers])
        for e in [self] + teachers:
            if e.model.scheduled_sampling and float(e.model.ss_prob) > 0.0:
                raise ValueError("scheduled sampling is live on %s (ss_prob %g): student and teachers would be fed different tokens"
                                 % ("the student" if e is self else "a teacher", float(e.model.ss_prob)))
        with _on_stream(self):
            return self._distill_training_epoch(dataloader, optimizer, criterion, teachers, tqdm_visible, rngs, alpha, temperature, weights)

    def _distill_training_epoch(self, dataloader, optimizer, criterion, teachers, tqdm_visible, rngs, alpha, temperature, weights):
        """_training_epoch with the teachers' forward passes in front of the student's and xe_backward_distill as the backward call"""
        from .distill import teacher_logits, xe_backward_distill
        for e in teachers:
            e.model.eval()
        self.last_distill_terms = []

        def begin(img_tensors, supp_info_datas, captions, lengths):
            t_feats = [e._features(e.modify_visual_inputs(img_tensors, supp_info_datas)) for e in teachers]
            t_logits = teacher_logits([e.model._handle() for e in teachers], t_feats, captions, lengths)

            def backward(h, grads, smoothing, n_glob):
                loss, hard, kd = xe_backward_distill(h, grads, t_logits, weights, alpha, temperature, smoothing, n_glob)
                self.last_distill_terms.append((hard, kd))
                return loss
            return backward
        return self._xe_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs, "Distillation Process", begin)

    # ---- E2 -------------------------------------------------------------------------------------------------
    # decoders whose SCST_training_epoch takes samples_per_image (BUTD, where the argument was introduced); the AoA and NIC engines
    # keep refusing it there and run the multi-sample step through SCST_multisample_training_epoch, which serves all three
    _multi_sample = True

    def SCST_training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=None, entropy_weight=0.0):
        """samples_per_image (beyond the reference): None = the reference's step (one sampled caption per image, greedy baseline);
        K = 2..8 = the multi-sample variant: K sampled captions per image, each baselined by the mean CIDEr-D of the other K - 1,
        no greedy rollout (BUTD decoders only).  entropy_weight > 0 (beyond the reference, both forms): the loss minus that multiple
        of the mean per-step entropy of the word distribution (scst_objective.py); 0 runs today's calls exactly.  ValueError for a
        bad argument before any device work."""
        if samples_per_image is not None:
            k = samples_per_image
            if not self._multi_sample:
                raise ValueError("samples_per_image: %s.SCST_training_epoch takes it for BUTD decoders only; call "
                                 "SCST_multisample_training_epoch(..., samples_per_image=K) or pass samples_per_image=None"
                                 % type(self).__name__)
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= 8:
                raise ValueError("samples_per_image must be None or an integer in 2..8, got %r" % (k,))
            samples_per_image = int(k)
        obj = _scst_objective_args(False, samples_per_image or 1, 1.0, entropy_weight)
        with _on_stream(self):
            return self._scst_training_epoch(dataloader, optimizer, criterion, tqdm_visible, rngs, samples_per_image, obj)

    def _scst_training_epoch(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=None, objective=None):
        """Engine.py:251-272: greedy baseline (eval mode) + multinomial rollout (train mode) + CIDEr-D reward +
        REINFORCE + clamp 0.25 + Adam, all on the device; `criterion` (RewardCriterion) is implied."""
        self.model.train()
        scorer = self.scorer()
        # References of images the scorer has not seen yet (the whole first epoch) are cooked on a loader thread one batch ahead
        # of the step that needs them (Utils.py:319-367 cooks them inside the step, for every batch of every epoch); a loader
        # that is not a prefetcher already is wrapped in one, which also stages host-side features through pinned buffers
        dataloader, restore = _cook_ahead(dataloader, scorer, self.device, getattr(self, "cook_ahead", True),
                                          self.__dict__.setdefault("_cook_cache", {}))
        monitor = _monitor(dataloader, "Training Process", tqdm_visible)
        losses = []
        try:
            self._scst_steps(monitor, scorer, optimizer, rngs, tqdm_visible, losses, samples_per_image, objective)
        finally:
            restore()
        return losses

    def _mark(self, marks):
        if marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)

    def phase_times(self, skip=0):
        """Mean GPU time per phase (ms) of the SCST steps recorded since `phase_events = []`: rollouts / reward / backward /
        allreduce_exposed (what the step WAITS for the gradient exchange behind its backward pass: 0 for one process, the whole
        all-reduce with dp_overlap off) / adam.  Call after a synchronize."""
        names = ("rollouts", "reward", "backward", "allreduce_exposed", "adam")
        steps = (self.phase_events or [])[skip:]
        if not steps:
            return {}
        return {n: sum(m[i].elapsed_time(m[i + 1]) for m in steps) / len(steps) for i, n in enumerate(names)}

    def _scst_steps(self, monitor, scorer, optimizer, rngs, tqdm_visible, losses, samples_per_image=None, objective=None):
        risk = objective is not None and objective.kind == "risk"
        for batch_i, (img_ids, img_tensors, img_gts, supp_info_datas) in enumerate(monitor):
            visual_inputs = self.modify_visual_inputs(img_tensors=img_tensors, supp_info_datas=supp_info_datas)
            feats = self._features(visual_inputs)
            h = self._hot_handle()
            rng = rngs[batch_i] if rngs is not None else self.model._next_rng()
            marks = [] if self.phase_events is not None else None
            self._mark(marks)
            if samples_per_image is None:
                greedy_res, seq_gen, seq_logprobs = h.rollouts(feats, 20, rng)
                self._mark(marks)
                rewards = scorer.reward(seq_gen, greedy_res, img_gts, img_ids)
            else:       # K sampled captions per image (rows img * K + k), each baselined by the mean reward of the other K - 1
                seq_gen, seq_logprobs = sample_n(h, feats, samples_per_image, 20, rng)
                self._mark(marks)
                rewards = scorer.reward_loo(seq_gen, samples_per_image, img_gts, img_ids, return_scores=risk)
            self._mark(marks)
            grads = self._grads()
            msum_glob = 0.0
            if icz_dist.is_distributed():
                ms = h.sample_mask_sum()
                if torch.is_tensor(ms) and hasattr(h, "set_mask_sum_global"):
                    # all-reduced on the device and handed over as a device scalar: no host round trip before backward
                    icz_dist.all_reduce_sum_(ms)
                    h.set_mask_sum_global(ms)
                    msum_glob = -1.0
                else:
                    msum_glob = icz_dist.all_reduce_scalar(ms)
            if risk:      # the objective divides by the image count of the whole step
                step_obj = objective.with_data(scores=rewards[1], n_img_global=icz_dist.all_reduce_scalar(float(len(img_ids)))
                                               if icz_dist.is_distributed() else 0.0)
            elif objective is not None:
                step_obj = objective.with_data(reward=rewards)
            ov = self._reduce_grads_begin(h)
            if objective is None:
                loss, _ = h.sample_backward(rewards, grads, msum_glob)
            else:
                loss3, _ = sample_backward_objective(h, step_obj, grads, msum_glob)
                loss = loss3[0:1]
                if self.scst_terms is not None:
                    self.scst_terms.append((loss3[1:2].clone(), loss3[2:3].clone()))
            self._mark(marks)
            self._reduce_grads_end(ov)
            self._mark(marks)
            self._apply(optimizer, 0.25)
            self._mark(marks)
            if marks is not None:
                self.phase_events.append(marks)
            losses.append(loss.clone())      # with graphs the handle returns one persistent buffer, overwritten by the next step
            if tqdm_visible:
                monitor.set_postfix(Loss=np.round(loss.item(), decimals=4))

    def _scst_distinct_training_epoch(self, dataloader, optimizer, tqdm_visible, rngs, n, estimator):
        """SCST_distinct_training_epoch's steps: sample_distinct, reward_loo's scores, make_batch, the training-mode forward,
        xe_backward_swor, then _scst_steps' tail"""
        from .stochastic_beam import sample_distinct
        from .swor import make_batch, swor_forward, xe_backward_swor
        self.model.train()
        scorer = self.scorer()
        dataloader, restore = _cook_ahead(dataloader, scorer, self.device, getattr(self, "cook_ahead", True),
                                          self.__dict__.setdefault("_cook_cache", {}))
        monitor = _monitor(dataloader, "Training Process", tqdm_visible)
        sta = self.caption_vocab.word2ix["<sta>"]
        losses, self.last_swor_stats = [], []
        try:
            for batch_i, (img_ids, img_tensors, img_gts, supp_info_datas) in enumerate(monitor):
                _check_distinct_batch(len(img_ids), n, self.model.max_rows, supp_info_datas)      # before the step's device work
                visual_inputs = self.modify_visual_inputs(img_tensors=img_tensors, supp_info_datas=supp_info_datas)
                feats = self._features(visual_inputs)
                h = self.model._handle()
                if rngs is not None:
                    s_rng, f_rng = rngs[batch_i]
                else:
                    f_rng = self.model._next_rng()
                    s_rng = icz_dist.seed_for_rank(self.model._seed)
                ids, lens, _fin, phi, G = sample_distinct(h, feats, n, 20, 1.0, s_rng)
                _, scores = scorer.reward_loo(ids, n, img_gts, img_ids, return_scores=True)
                batch = make_batch(ids, lens, sta, n)
                swor_forward(h, feats, batch, f_rng)
                grads = self._grads()
                n_glob = icz_dist.all_reduce_scalar(float(len(img_ids))) if icz_dist.is_distributed() else 0.0
                ov = self._reduce_grads_begin(h)
                (loss, _by_image), stats = xe_backward_swor(h, grads, phi, G, scores, batch, estimator, n_glob)
                self._reduce_grads_end(ov)
                self._apply(optimizer, 0.25)
                self.last_swor_stats.append(stats)
                losses.append(loss.clone())
                if tqdm_visible:
                    monitor.set_postfix(Loss=np.round(loss.item(), decimals=4))
        finally:
            restore()
        return losses

    # ---- E3 -------------------------------------------------------------------------------------------------
    def eval_captions_json_generation(self, dataloader, eval_beam_size=-1, tqdm_visible=True, *, length_penalty=None, block_ngram=0,
                                      beam_groups=1, diversity=0.0):
        """length_penalty / block_ngram (an extension, beam search only; include/icz.h: icz_beam_opts): rank the finished beams by
        a length-penalised score (None, ('avg' | 'wu', alpha), 'avg_<alpha>', 'wu_<alpha>') and forbid repeated n-grams.
        beam_groups / diversity (beam search only; icz_beam_diversity): diverse beam search with eval_beam_size / beam_groups
        beams per group; the JSON holds each image's rank-0 hypothesis."""
        opts = _check_beam_opts(eval_beam_size, length_penalty, block_ngram, beam_groups, diversity, False)
        return _eval_captions([self], None, False, dataloader, eval_beam_size, tqdm_visible, opts)

    def constrained_captions_json_generation(self, dataloader, constraints, eval_beam_size=3, tqdm_visible=True, *, length_penalty=None,
                                             block_ngram=0):
        """Captions that must contain given words (an extension; include/icz.h: icz_beam_constraints, constrained.py): constrained beam
        search with eval_beam_size beams per set of satisfied constraints.  constraints: {image id: [constraint, ...]}, a constraint
        a word or a list of alternative words (up to 3 constraints of up to 4 words each); an image that is absent is unconstrained,
        out-of-vocabulary alternatives are dropped and a constraint left without a word counts as unsatisfied.  Returns the JSON list
        of eval_captions_json_generation with "satisfied" added: one boolean per constraint of the image, in the order given.  Sharded
        over the ranks and gathered the same way; a batch above the handle's row capacity / (2^C * eval_beam_size) is decoded in
        chunks.  With an empty dict the captions are eval_captions_json_generation's at that beam size.  Bad arguments raise
        ValueError before any device work."""
        return _constrained_captions_json_generation([self], None, False, dataloader, constraints, eval_beam_size, tqdm_visible, length_penalty,
                                                     block_ngram)

    def sample_captions_json_generation(self, dataloader, samples_per_image=1, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                                        tqdm_visible=True):
        """Sampled captions for evaluation (an extension; include/icz.h: icz_*_sample_decode): `samples_per_image` (1..8) captions
        per image drawn in evaluation mode from softmax(logits / temperature) restricted to the top_k largest tokens (0 = off) and
        the nucleus of mass top_p (1 = off), 20 steps as the greedy evaluation.  Returns {"image_id", "caption", "score"} entries,
        samples_per_image per image in loader order; score = the model's summed log-probability of the caption's tokens.  Batch i
        of the loader draws from Philox seed `seed * 2**20 + i`: one seed gives the same captions run to run.  Sharded over the
        ranks and gathered as eval_captions_json_generation does.  Bad arguments raise ValueError before any device work."""
        _check_sample_args(self, samples_per_image, temperature, top_k, top_p, seed)
        return _sample_captions([self], None, False, dataloader, int(samples_per_image), temperature, top_k, top_p, seed, tqdm_visible)

    # ---- caption sets: consensus reranking and the set report (an extension; caption_sets.py, include/icz.h "Caption sets") -------
    def _pack_set(self, entries, samples_per_image):
        from . import caption_sets as cs
        ids, caps = cs.group_entries(entries, samples_per_image)
        word2ix = self.caption_vocab.word2ix
        for grp in caps:                       # every ValueError before any device work: pack_candidates raises the same ones
            for cap in grp:
                words = cap.split()
                if len(words) > cs.MAX_TOKENS:
                    raise ValueError("caption with %d words: the device scorer handles at most %d" % (len(words), cs.MAX_TOKENS))
                for w in words:
                    if w not in word2ix:
                        raise ValueError("word %r is not in the vocabulary" % (w,))
        _check_cider_df(self)
        return ids, caps, lambda: cs.pack_candidates(caps, word2ix, self.device)

    def rerank_captions_json(self, entries, samples_per_image):
        """Consensus (minimum-Bayes-risk) reranking of a caption set: entries = the output of sample_captions_json_generation, or any
        list of {"image_id", "caption"[, "score"]} with samples_per_image (2..8) consecutive entries per image.  Of every image the
        caption that agrees most with its siblings is kept: the one with the largest CIDEr-D against the other samples_per_image - 1
        captions as references (on the scorer's df table; ties: the first).  Returns one {"image_id", "caption", "score",
        "consensus"} per image in entry order -- "score" is the kept entry's own (None without one) -- which
        coco_eval.evaluate_captions takes as it is.  Bad arguments raise ValueError before any device work."""
        ids, caps, pack = self._pack_set(entries, samples_per_image)
        entries = list(entries)
        K = int(samples_per_image)
        with _on_stream(self):
            _, cons, best = self.scorer().pairwise(pack(), K)
            cons, best = cons.cpu().numpy(), best.cpu().numpy()
        out = []
        for i, image_id in enumerate(ids):
            e = entries[i * K + int(best[i])]
            out.append({"image_id": image_id, "caption": e["caption"], "score": e.get("score"), "consensus": float(cons[i, best[i]])})
        return out

    def consensus_captions_json_generation(self, dataloader, samples_per_image=5, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                                           tqdm_visible=True):
        """sample_captions_json_generation (same arguments, samples_per_image 2..8) followed by rerank_captions_json: one consensus
        caption per image."""
        from .caption_sets import check_k
        check_k(samples_per_image, 2)
        _check_cider_df(self)
        entries = self.sample_captions_json_generation(dataloader, samples_per_image, temperature, top_k, top_p, seed, tqdm_visible)
        return self.rerank_captions_json(entries, samples_per_image)

    def sample_distinct_captions_json_generation(self, dataloader, samples_per_image=5, temperature=1.0, seed=0, tqdm_visible=True):
        """Captions sampled WITHOUT replacement (an extension; include/icz.h: icz_*_sample_distinct, stochastic_beam.py): stochastic
        beam search returns `samples_per_image` (1..8) distinct captions per image that are exactly a sample without replacement from
        softmax(logits / temperature) over whole captions, 20 steps, for the cost of one beam search of that width.  Returns
        {"image_id", "caption", "score", "perturbed"} entries, samples_per_image per image in loader order, an image's entries sorted
        by "perturbed" descending; score = the caption's summed log-probability under the tempered distribution, perturbed = its
        Gumbel-perturbed value G (float64; what the without-replacement estimators of Kool et al., ICLR 2020, take).  Batch i of the
        loader draws from Philox seed `seed * 2**20 + i`; a batch above the handle's row capacity / samples_per_image is decoded in
        chunks that draw the whole batch's noise (chunked = whole); sharded over the ranks and gathered as
        sample_captions_json_generation does.  "caption" ends at <end> or at the first <pad> (0): a hypothesis that sampled <pad> as a
        token prints up to there while its score is the whole sequence's, and two distinct hypotheses may then print alike (a trained
        model gives <pad> no mass to speak of).  An image with fewer than samples_per_image sequences in all has its empty slots dropped -- this cannot happen at a
        real vocabulary (V^20 sequences).  Bad arguments raise ValueError before any device work."""
        return _sample_distinct_captions_json_generation([self], None, False, dataloader, samples_per_image, temperature, seed, tqdm_visible)

    def consensus_distinct_captions_json_generation(self, dataloader, samples_per_image=5, temperature=1.0, seed=0, tqdm_visible=True):
        """sample_distinct_captions_json_generation (same arguments, samples_per_image 2..8) followed by rerank_captions_json: one
        consensus caption per image, voted by distinct candidates."""
        from .caption_sets import check_k
        check_k(samples_per_image, 2)
        _check_cider_df(self)
        entries = self.sample_distinct_captions_json_generation(dataloader, samples_per_image, temperature, seed, tqdm_visible)
        return self.rerank_captions_json(entries, samples_per_image)

    def caption_set_report(self, entries, samples_per_image, gts):
        """The report of a caption set in the style of self-critical.pytorch's eval_multi.  entries as for rerank_captions_json,
        gts = {image id: [reference strings]} holding every image of the entries.  Returns
          oracle_CIDErD / mean_CIDErD / picked_CIDErD  mean over the images of the best / the mean / the consensus pick's CIDEr-D against
                                           the references, on the scorer's df table -- the SCST reward's scale, not the corpus CIDEr
                                           of coco_eval;
          Div_1, Div_2                     distinct n-grams / total words of an image's set (caption_sets.div_n);
          mBleu_1 .. mBleu_4               corpus BLEU of every caption against its siblings (caption_sets.mbleu);
          pairwise_CIDErD                  mean off-diagonal CIDEr-D between an image's captions (caption_sets.mean_pairwise).
        Bad arguments raise ValueError before any device work."""
        from . import caption_sets as cs
        ids, caps, pack = self._pack_set(entries, samples_per_image)
        if not hasattr(gts, "__getitem__") or not hasattr(gts, "__contains__"):
            raise ValueError("gts must map image ids to lists of reference strings")
        for i in ids:
            if i not in gts or len(gts[i]) == 0:
                raise ValueError("image %r has no references in gts" % (i,))
        K = int(samples_per_image)
        with _on_stream(self):
            cands = pack()
            scorer = self.scorer()
            pair, _, best = scorer.pairwise(cands, K)
            pair, best = pair.cpu().numpy(), best.cpu().numpy().astype(np.int64)
            scores = scorer.scores_csr(cands, K, gts, ids).cpu().numpy()
            counts = cs.ngram_counts(cands)
            mb = cs.mbleu(cands)
        rep = {"oracle_CIDErD": float(np.mean(scores.max(axis=1))), "mean_CIDErD": float(np.mean(scores)),
               "picked_CIDErD": float(np.mean(scores[np.arange(len(ids)), best])),
               "Div_1": cs.div_n(counts, 1), "Div_2": cs.div_n(counts, 2)}
        for k in range(4):
            rep["mBleu_%d" % (k + 1)] = mb[k]
        rep["pairwise_CIDErD"] = cs.mean_pairwise(pair)
        return rep


    # ---- scoring given captions (an extension; scoring.py, include/icz.h: icz_*_score_captions) ---------------------------------
    def score_captions_json(self, dataloader, entries, captions_per_image=1, tqdm_visible=True):
        """The model's log-probability of captions it is handed.  entries: {"image_id", "caption", ...} with captions_per_image
        (1..8) consecutive entries per image, images in loader order -- what sample_captions_json_generation returns; dataloader: the
        evaluation loader (image_ids, img_tensors, supp_info_datas).  The words go through the vocabulary's <unk> fallback and
        <end> is appended.  Returns the entries in order, each extended by "logprob" (the summed log-probability, float), "tokens"
        (scored tokens, <end> included) and "logprobs" (one per token).  A group whose image_id is not the loader's raises
        ValueError; every argument error that needs no device is raised before the first batch.  A batch of more than
        (row capacity // captions_per_image) images is scored in chunks of images.  Not sharded: under torch.distributed every
        rank scores everything."""
        entries, n = _check_score_entries(entries, captions_per_image)
        with _on_stream(self):
            return _score_entries([self], None, dataloader, entries, n, tqdm_visible)

    def rescore_captions_json(self, dataloader, entries, captions_per_image, length_penalty=None, tqdm_visible=True):
        """Likelihood reranking: score_captions_json, then of every image the caption with the largest length-penalised
        log-probability (length_penalty: None, ('avg' | 'wu', alpha), 'avg_<alpha>', 'wu_<alpha>' as beam search's, on the scored
        tokens with <end> counted, so at least one; ties: the first).  Returns one {"image_id", "caption", "logprob", "rank_score"} per image in
        entry order, which coco_eval.evaluate_captions takes as it is.  Not sharded: every rank scores everything."""
        lp = parse_length_penalty(length_penalty)            # a bad penalty raises here, before any device work
        entries, n = _check_score_entries(entries, captions_per_image)
        with _on_stream(self):
            scored = _score_entries([self], None, dataloader, entries, n, tqdm_visible)
        return _pick_by_likelihood(scored, n, lp)

    def reference_perplexity(self, dataloader, tqdm_visible=True):
        """The perplexity of a split's reference captions under the model (self-critical.pytorch's eval_split reports it beside
        CIDEr).  dataloader: the SCST loader (img_ids, img_tensors, img_gts, supp_info_datas) with img_gts[image id] = the image's
        reference strings.  Every reference of every image is scored; an image with fewer references than its batch's maximum gets
        empty captions, which score nothing; more than 8 references per image are scored in groups of 8.  Returns {"ppl",
        "nll_per_token", "tokens", "captions"}: ppl = exp(-sum of log-probabilities / tokens), <end> counted, summed in float64 on
        the host.  Not sharded: every rank scores everything."""
        with _on_stream(self):
            return _reference_perplexity(self, dataloader, tqdm_visible)


class AoADetection_Eng(BUTDDetection_Eng):
    """ModelEngines/AoA_Engine.py (same visual-input handling as the BUTD engine) + the three hot Engine methods.
    `use_bu='adaptive'` (10..100 boxes per image, Main.py:158): the handle is sized for 100 regions and every batch carries
    its region counts (AoA_Engine.py:37-46 builds the equivalent prefix masks)."""

    # the AoA library's callback stages (include/icz.h: icz_aoa_set_grad_callback): 41 MB + 92 MB of the 163 MB of decoder gradients are
    # on the wire before the backward call returns; the attention block and h_norm (30 MB) follow after it
    _multi_sample = False
    _grouped_xe = False
    _GRAD_STAGES = (("decoder.predict.weight_v", "decoder.predict.weight_g", "decoder.predict.bias"),
                    ("decoder.embed.0.weight", "decoder.lstm.weight_ih", "decoder.lstm.weight_hh", "decoder.lstm.bias_ih", "decoder.lstm.bias_hh"))

    def __init__(self, *args, train_refiner=False, **kwargs):
        """train_refiner (beyond the reference, which optimises the decoder only): also fit aoa_refine.* and img_feats_porjection.*."""
        super().__init__(*args, **kwargs)
        self.train_refiner = train_refiner

    @property
    def train_refiner(self):
        return self.model.train_refiner

    @train_refiner.setter
    def train_refiner(self, on):
        on = bool(on)
        if on != self.model.train_refiner:
            self.model.train_refiner = on         # pushed to the handle as its option by the next _handle()
            self._flat = None                      # the flat gradient buffer gains / loses the refiner's slice
            self._hooked = None

    def model_construction(self, max_batch):
        from .aoa import AoADetection_Captioner
        s = self.settings
        assert s["model_type"] in ("AoADetection", "AoASpatial")
        regions = s.get("num_regions", 100 if self.use_bu == "adaptive" else 36)
        return AoADetection_Captioner(vocab_size=len(self.caption_vocab), num_heads=s.get("num_heads", 8), hidden_dim=s["hidden_dim"],
                                      embed_dim=s["embed_dim"], device=str(self.device), num_regions=regions,
                                      enc_dim=s.get("enc_dim", 2048), max_batch=max_batch)


class NIC_Eng(BUTDDetection_Eng):
    """ModelEngines/NIC_Engine.py (= the base Engine) with the three hot methods on the NIC decoder handle.  The CNN encoder +
    img_embedding of NIC_Model.py:8-37 is outside the path: batches carry the image embedding -- `supp_info_datas =
    {'img_feats': (B, embed_dim) tensor}` -- or the Captioner was given an `encoder` module for `img_tensors`."""

    _multi_sample = False
    _grouped_xe = False

    def model_construction(self, max_batch):
        from .nic import NICDecoder_Captioner
        s = self.settings
        assert s["model_type"] == "NIC"
        return NICDecoder_Captioner(embed_dim=s["embed_dim"], hidden_dim=s["hidden_dim"], vocab_size=len(self.caption_vocab),
                                    device=str(self.device), max_batch=max_batch)

    def modify_visual_inputs(self, img_tensors, supp_info_datas=None):
        if isinstance(supp_info_datas, dict) and torch.is_tensor(supp_info_datas.get("img_feats")):
            return {"img_feats": supp_info_datas["img_feats"].to(self.device, torch.float32)}
        return {"img_tensors": img_tensors.to(self.device)}            # Engine.py:32-41


class BUTDSpatial_Eng(BUTDDetection_Eng):
    """Same decoder over a 7x7x2048 grid fed as precomputed features (49 regions); the CNN encoder of
    BUTD_Model.py:8-38 is outside the hot path."""

    def model_construction(self, max_batch):
        self.settings.setdefault("num_regions", self.settings.get("enc_img_size", 7) ** 2)
        return super().model_construction(max_batch)


class _on_stream:
    """Run a block on the engine's stream, ordered after / before the caller's current stream."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.outer = torch.cuda.current_stream(self.eng.device)
        self.eng.stream.wait_stream(self.outer)
        self.ctx = torch.cuda.stream(self.eng.stream)
        self.ctx.__enter__()

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        self.outer.wait_stream(self.eng.stream)
        return False


def _rank_batches(loader, rank, world):
    """(batch index, batch) of the batches i with i % world == rank, loading as little else as the loader allows."""
    if hasattr(loader, "shard"):
        for i, b in loader.shard(rank, world):
            yield i, b
    elif hasattr(loader, "__getitem__") and hasattr(loader, "__len__"):
        for i in range(rank, len(loader), world):
            yield i, loader[i]
    else:
        for i, b in enumerate(loader):
            if i % world == rank:
                yield i, b


def _cook_ahead(loader, scorer, device, enabled, cache=None):
    """-> (loader whose worker thread cooks unseen references one batch ahead, restore()).  `cache` (a dict the Engine keeps) holds
    the wrapping prefetcher across epochs: its pinned ring, copy stream and thread pool are set up once."""
    from .features import DevicePrefetcher
    cook = lambda batch: scorer.prepare(batch[0], batch[2])
    if not enabled:
        return loader, lambda: None
    if isinstance(loader, DevicePrefetcher):
        if loader.on_batch is not None:
            return loader, lambda: None
        loader.on_batch = cook

        def restore():
            loader.on_batch = None
        return loader, restore
    pf = cache.get("pf") if cache is not None else None
    if pf is None:
        pf = DevicePrefetcher(loader, device, on_batch=cook)
        if cache is not None:
            cache["pf"] = pf
    pf.loader, pf.on_batch = loader, cook

    def release():
        pf.loader = None            # do not keep the caller's loader alive between epochs
    return pf, release


def _monitor(dataloader, desc, visible):
    if not visible:
        return dataloader
    import tqdm
    return tqdm.tqdm(dataloader, desc=desc)


# ---- what the caption-generation and scoring paths share: the batch walk, the gathered rows, the chunks, the checks ---------------
def _prepare(engines, weights, ensemble, ens, img_tensors, supp_info_datas):
    """One loader batch under the one engine or (ensemble) the ensemble of the engines: every engine turns it into its own features
    and hands out its hot handle -> (the handle to call, its features -- a list of one per member for the ensemble --, the
    EnsembleHandle to keep for the next batch: it is rebuilt only when a member's handle is another object)."""
    feats = [e._features(e.modify_visual_inputs(img_tensors=img_tensors, supp_info_datas=supp_info_datas)) for e in engines]
    handles = [e._hot_handle() for e in engines]
    if not ensemble:
        return handles[0], feats[0], None
    from .ensemble import EnsembleHandle
    if ens is None or any(a is not b for a, b in zip(ens.handles, handles)):
        ens = EnsembleHandle(handles, weights)
    return ens, feats, ens


def _batches(engines, weights, ensemble, dataloader, desc, tqdm_visible, shard=True):
    """The batch walk of every generation and scoring path: the engines go into evaluation mode now, and the generator returned
    hands out (batch index, image ids, handle, features) per batch of the evaluation loader (_prepare).  Data-parallel with `shard`
    (torch.distributed initialised): this rank's batches only, i % world == rank.  An indexable loader (list,
    Dataset-like: __len__ + __getitem__) or one with a shard(rank, world) method is never asked for the other ranks' batches (no
    feature I/O for them); any other iterable is walked in full and the foreign batches dropped (_rank_batches)."""
    for e in engines:
        e.model.eval()
    if not shard:
        numbered = enumerate(_monitor(dataloader, desc, tqdm_visible))
    elif icz_dist.is_distributed():
        numbered = _monitor(_rank_batches(dataloader, icz_dist.rank(), icz_dist.world_size()), desc, tqdm_visible)
    else:
        numbered = _monitor(enumerate(dataloader), desc, tqdm_visible)

    def walk():
        ens = None
        for batch_i, (image_ids, img_tensors, supp_info_datas) in numbered:
            h, feats, ens = _prepare(engines, weights, ensemble, ens, img_tensors, supp_info_datas)
            yield batch_i, image_ids, h, feats
    return walk()


class _Rows:
    """The rows a rank decoded, each with its image id and its place in the loader: key = (batch index << 20) + row index within
    the batch.  gathered(): (image id, row) of ALL ranks in loader order -- what the corpus-level scorer after it
    (COCO_Eval_Utils.py:15-35) needs in one place; every rank gets the complete list, rank 0 is the one that should write / score it."""

    def __init__(self):
        self.ids, self.rows, self.keys = [], [], []

    def add(self, batch_i, j, image_id, row):
        self.ids.append(int(image_id))
        self.rows.append(row)
        self.keys.append((batch_i << 20) + j)

    def gathered(self, device):
        if icz_dist.is_distributed():
            return zip(*icz_dist.gather_caption_rows(self.keys, self.ids, self.rows, device))
        return zip(self.ids, self.rows)


def _slice_feats(f, lo, hi):
    from .regions import RegionBatch
    if isinstance(f, RegionBatch):
        return RegionBatch(f.feats[lo:hi], None if f.counts is None else list(f.counts)[lo:hi])
    return f[lo:hi]


def _chunks(feats, ensemble, n_img, per, refuse=None, limit=None, whole=False):
    """A batch of n_img images in calls of at most `per` (and at most `limit`) images -> (lo, hi, the features of images lo..hi).
    Where not even one image fits (per < 1): ValueError(refuse), or one image per call without a `refuse`.  whole: a batch that
    fits one call is handed over unsliced."""
    if per < 1:
        if refuse is not None:
            raise ValueError(refuse)
        per = 1
    if limit is not None:
        per = min(per, limit)
    for lo in range(0, n_img, per):
        hi = min(n_img, lo + per)
        if whole and per >= n_img:
            yield lo, hi, feats
        else:
            yield lo, hi, [_slice_feats(f, lo, hi) for f in feats] if ensemble else _slice_feats(feats, lo, hi)


_words = CaptionerBase._words      # a row of ids -> its words up to <end> (stop_at_pad: or up to the first <pad>), without <sta>


def _pack_row(ids, score, perturbed=None):
    """Token ids with a float32 score and, if given, a float64 perturbed value behind them as their bit patterns: one uint32, then
    two uint32 halves, low then high -- non-negative integers, which is what gather_caption_rows carries."""
    tail = [int(score.view(np.uint32))]
    if perturbed is not None:
        bits = int(perturbed.view(np.uint64))
        tail += [bits & 0xFFFFFFFF, bits >> 32]
    return np.concatenate([ids, tail])


def _unpack_row(row, perturbed=False):
    """_pack_row back -> (ids, score) or (ids, score, perturbed value), bit for bit"""
    tail = 3 if perturbed else 1
    score = float(np.array([int(row[-tail])], dtype=np.uint32).view(np.float32)[0])
    if not perturbed:
        return row[:-1], score
    return row[:-3], score, float(np.array([int(row[-2]) | (int(row[-1]) << 32)], dtype=np.uint64).view(np.float64)[0])


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
        raise ValueError("seed %r is not a non-negative integer" % (seed,))


def _check_sample_args(lead, samples_per_image, temperature, top_k, top_p, seed):
    make_sample_opts(temperature, top_k, top_p, samples_per_image)
    _check_seed(seed)
    if top_k > len(lead.caption_vocab):
        raise ValueError("top_k %d above the vocabulary size %d" % (top_k, len(lead.caption_vocab)))


def _check_cider_df(eng):
    if eng._cider_df is None and eng._scorer is None:
        raise ValueError("caption sets are scored with CIDEr-D: the engine needs cider_df (the document-frequency table)")


def _check_beam_opts(eval_beam_size, length_penalty, block_ngram, beam_groups, diversity, ensemble):
    """The beam options of eval_captions_json_generation (checked where one is set) and eval_ensemble_captions_json_generation
    (always checked, the beam size with them) -> (length_penalty, block_ngram, beam_groups, diversity) for beam_search_opts, or None
    for the single model without an option: the plain beam_search.  A bad option raises here, before any device work."""
    diverse = isinstance(beam_groups, bool) or isinstance(diversity, bool) or beam_groups != 1 or diversity != 0.0
    given = length_penalty is not None or bool(block_ngram) or diverse
    if given and eval_beam_size == -1:
        raise ValueError("length_penalty / block_ngram / beam_groups / diversity need beam search (eval_beam_size != -1)")
    if not given and not ensemble:
        return None
    parse_length_penalty(length_penalty)
    if int(block_ngram) not in (0, 2, 3, 4):
        raise ValueError("block_ngram %d not 0, 2, 3 or 4" % int(block_ngram))
    if eval_beam_size != -1:
        if ensemble and (isinstance(eval_beam_size, bool) or not isinstance(eval_beam_size, int) or eval_beam_size < 1):
            raise ValueError("eval_beam_size %r: -1 (greedy) or a beam size >= 1" % (eval_beam_size,))
        make_diversity(beam_groups, diversity, eval_beam_size)      # groups not dividing the beam, bad diversity
    return length_penalty, int(block_ngram), int(beam_groups), float(diversity)


def _ensemble_engine_checks(engines, weights):
    """the engine checks of eval_ensemble_captions_json_generation -> the engines as a list"""
    from .ensemble import check_members, check_weights
    engines = list(engines)
    check_members(len(engines))
    if len({len(e.caption_vocab) for e in engines}) != 1:
        raise ValueError("the engines' vocabularies differ in size %s" % [len(e.caption_vocab) for e in engines])
    if len({str(e.device) for e in engines}) != 1:
        raise ValueError("the engines sit on different devices %s" % [str(e.device) for e in engines])
    check_weights(weights, len(engines))
    return engines


# ---- greedy / beam evaluation ---------------------------------------------------------------------------------------------------
def _eval_captions(engines, weights, ensemble, dataloader, eval_beam_size, tqdm_visible, opts):
    """Engine.py:274-300 under the one engine or (ensemble) the ensemble of the engines.  Beam search accepts any batch size here
    (the reference's loader uses 1); opts: _check_beam_opts.  Data-parallel: rank r decodes the batches i with i % world == r
    (_batches), the (image id, token ids) rows are all-gathered and every rank returns the complete list in loader order (_Rows)."""
    lead = engines[0]
    with _on_stream(lead):
        batches = _batches(engines, weights, ensemble, dataloader, "Generating Process", tqdm_visible)
        print("Generating captions json for evaluation%s. Beam Search: %s" % (" (ensemble of %d)" % len(engines) if ensemble else "",
                                                                                eval_beam_size != -1))
        out = _Rows()
        for batch_i, image_ids, h, feats in batches:
            if eval_beam_size != -1 and opts is not None:
                seqs, lens, _ = h.beam_search_opts(feats, eval_beam_size, 50, 1, *opts)
                seqs, lens = seqs[:, 0].cpu().numpy(), lens[:, 0].cpu().numpy()
                rows = [seqs[i, :lens[i]] for i in range(len(lens))]
            elif eval_beam_size != -1:
                seqs, lens = h.beam_search(feats, eval_beam_size, 50)
                seqs, lens = seqs.cpu().numpy(), lens.cpu().numpy()
                rows = [seqs[i, :lens[i]] for i in range(len(lens))]
            else:
                rows = list(h.greedy(feats, 20).cpu().numpy())
            for j, image_id in enumerate(image_ids):
                out.add(batch_i, j, image_id, rows[j])
        pairs = out.gathered(lead.device)
    return [{"image_id": image_id, "caption": " ".join(_words(row, lead.caption_vocab))} for image_id, row in pairs]


def eval_ensemble_captions_json_generation(engines, dataloader, eval_beam_size=-1, tqdm_visible=True, *, weights=None, length_penalty=None,
                                           block_ngram=0, beam_groups=1, diversity=0.0):
    """Engine.eval_captions_json_generation for an ensemble of 1..4 engines (BUTD / AoA / NIC) of one vocabulary (an extension;
    include/icz.h: icz_ensemble_*): every engine turns the shared batch into its own features (its modify_visual_inputs and
    _features), the members decode together on the averaged word probabilities (`weights`: None = uniform), greedy or with beam
    search and its options.  Returns the JSON list of the single-model method (the first engine's vocabulary), sharded over the
    ranks and all-gathered in loader order the same way.  Arguments are checked before any device work (ValueError)."""
    engines = _ensemble_engine_checks(engines, weights)
    opts = _check_beam_opts(eval_beam_size, length_penalty, block_ngram, beam_groups, diversity, True)
    return _eval_captions(engines, weights, True, dataloader, eval_beam_size, tqdm_visible, opts)


# ---- constrained beam search ----------------------------------------------------------------------------------------------------
def _constrained_captions_json_generation(engines, weights, ensemble, dataloader, constraints, beam, tqdm_visible, length_penalty, block_ngram,
                                          max_chunk=None):
    """The constrained search of Engine.constrained_captions_json_generation under the one engine or (ensemble) the ensemble of the
    engines.  max_chunk (tests): at most that many images per call."""
    from . import constrained as cst
    lead = engines[0]
    if not isinstance(constraints, dict):
        raise ValueError("constraints must map image ids to lists of constraints, got %s" % type(constraints).__name__)
    parse_length_penalty(length_penalty)
    if int(block_ngram) not in (0, 2, 3, 4):
        raise ValueError("block_ngram %d not 0, 2, 3 or 4" % int(block_ngram))
    # every image's words -> ids now, so that a bad constraint is refused before the first batch is decoded
    given = {int(k): [[c] if isinstance(c, str) else list(c) for c in (v or [])] for k, v in constraints.items()}
    keys = list(given)
    enc, dropped = cst.encode_constraints([given[k] for k in keys], lead.caption_vocab)
    packed = cst.make_constraints(enc, len(keys), len(lead.caption_vocab))
    cst.check_beam(beam, packed.shape[1])
    lost = {}
    for img, q, _ in dropped:
        lost.setdefault(keys[img], set()).add(q)
    ids_of = dict(zip(keys, enc))
    with _on_stream(lead):
        out = _Rows()
        for batch_i, image_ids, h, feats in _batches(engines, weights, ensemble, dataloader, "Generating Process", tqdm_visible):
            nb = len(image_ids)
            words = cst.make_constraints([ids_of.get(int(i), []) for i in image_ids], nb, h.V)
            # One C for the whole batch: a chunk with a constrained image searches the states the batch does.  A chunk without any
            # (as a batch without any) is the plain options search on eval_beam_size rows per image, which is what an unconstrained
            # image's state 0 runs inside a constrained call; its caption is the same as far as the decoder's GEMMs agree between
            # the two row counts (they do on every case tested), not by construction.
            need = cst.rows_per_image(words, beam)
            refuse = "one image takes %d rows, the handle's row capacity is %d" % (need, h.max_rows)
            for lo, hi, part in _chunks(feats, ensemble, nb, h.max_rows // need, refuse, max_chunk):
                seqs, lens, _, sat = cst.beam_search(h, part, words[lo:hi], beam, 50, 1, length_penalty, int(block_ngram))
                seqs, lens, sat = seqs[:, 0].cpu().numpy(), lens[:, 0].cpu().numpy(), sat[:, 0].cpu().numpy()
                for i in range(hi - lo):      # the state rides behind the tokens through the gather
                    out.add(batch_i, lo + i, image_ids[lo + i], np.concatenate([seqs[i, :lens[i]], [np.float32(sat[i])]]))
        pairs = out.gathered(lead.device)
    result = []
    for image_id, row in pairs:
        sat, q, flags = int(row[-1]), 0, []
        for c in range(len(given.get(image_id, []))):          # a dropped constraint took no bit
            if c in lost.get(image_id, ()):
                flags.append(False)
            else:
                flags.append(bool((sat >> q) & 1))
                q += 1
        result.append({"image_id": image_id, "caption": " ".join(_words(row[:-1], lead.caption_vocab)), "satisfied": flags})
    return result


def constrained_ensemble_captions_json_generation(engines, dataloader, constraints, eval_beam_size=3, tqdm_visible=True, *, weights=None,
                                                  length_penalty=None, block_ngram=0):
    """Engine.constrained_captions_json_generation for an ensemble of 1..4 engines (BUTD / AoA / NIC) of one vocabulary: the members
    decode together on the averaged word probabilities (`weights`: None = uniform); the first engine's vocabulary encodes the
    constraints and words the captions."""
    engines = _ensemble_engine_checks(engines, weights)
    return _constrained_captions_json_generation(engines, weights, True, dataloader, constraints, eval_beam_size, tqdm_visible, length_penalty,
                                                 block_ngram)


# ---- sampled captions -----------------------------------------------------------------------------------------------------------
def _sample_captions(engines, weights, ensemble, dataloader, n, temperature, top_k, top_p, seed, tqdm_visible):
    """Engine.sample_captions_json_generation under the one engine or (ensemble) the ensemble of the engines"""
    lead = engines[0]
    with _on_stream(lead):
        out = _Rows()
        for batch_i, image_ids, h, feats in _batches(engines, weights, ensemble, dataloader, "Sampling Process", tqdm_visible):
            ids, _, score = h.sample_decode(feats, n, 20, temperature, top_k, top_p, (seed << 20) + batch_i)
            ids, score = ids.cpu().numpy(), score.cpu().numpy()
            for r in range(ids.shape[0]):                              # loader order: batch index, then image, then sample
                out.add(batch_i, r, image_ids[r // n], _pack_row(ids[r], score[r]))
        pairs = out.gathered(lead.device)
    result = []
    for image_id, row in pairs:
        ids, score = _unpack_row(row)
        result.append({"image_id": image_id, "caption": " ".join(_words(ids, lead.caption_vocab, True)), "score": score})
    return result


def sample_ensemble_captions_json_generation(engines, dataloader, samples_per_image=1, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                                             tqdm_visible=True, *, weights=None):
    """Engine.sample_captions_json_generation for an ensemble of 1..4 engines (BUTD / AoA / NIC) of one vocabulary (an extension;
    include/icz.h: icz_ensemble_sample_decode): every engine turns the shared batch into its own features, and `samples_per_image`
    (1..8) captions per image are drawn from the averaged word probabilities (`weights`: None = uniform) under temperature / top_k /
    top_p, 20 steps.  Returns {"image_id", "caption", "score"} entries, samples_per_image per image in loader order (the first
    engine's vocabulary); score = the ensemble's summed log-probability of the caption's tokens.  Batch i draws from Philox seed
    `seed * 2**20 + i`; sharded over the ranks and gathered as the single-model method.  Arguments are checked before any device
    work (ValueError)."""
    engines = _ensemble_engine_checks(engines, weights)
    _check_sample_args(engines[0], samples_per_image, temperature, top_k, top_p, seed)
    return _sample_captions(engines, weights, True, dataloader, int(samples_per_image), temperature, top_k, top_p, seed, tqdm_visible)


def consensus_ensemble_captions_json_generation(engines, dataloader, samples_per_image=5, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                                                tqdm_visible=True, *, weights=None):
    """sample_ensemble_captions_json_generation (same arguments, samples_per_image 2..8) followed by the first engine's
    rerank_captions_json: one consensus caption per image."""
    from .caption_sets import check_k
    engines = _ensemble_engine_checks(engines, weights)
    check_k(samples_per_image, 2)
    lead = engines[0]
    _check_sample_args(lead, samples_per_image, temperature, top_k, top_p, seed)         # every option error in front of the engines' state
    _check_cider_df(lead)
    entries = sample_ensemble_captions_json_generation(engines, dataloader, samples_per_image, temperature, top_k, top_p, seed, tqdm_visible,
                                                       weights=weights)
    return lead.rerank_captions_json(entries, samples_per_image)


# ---- sampling without replacement -----------------------------------------------------------------------------------------------
def _sample_distinct_captions_json_generation(engines, weights, ensemble, dataloader, samples_per_image, temperature, seed, tqdm_visible):
    """Engine.sample_distinct_captions_json_generation over one engine's own handle, or (ensemble) an EnsembleHandle over the engines'"""
    from . import stochastic_beam as sbs
    lead = engines[0]
    n, _, temperature = sbs.check_args(samples_per_image, 20, temperature, len(lead.caption_vocab))
    _check_seed(seed)
    with _on_stream(lead):
        out = _Rows()
        for batch_i, image_ids, h, feats in _batches(engines, weights, ensemble, dataloader, "Sampling Process", tqdm_visible):
            # a batch above the row capacity / n is decoded in chunks of images; a chunk draws the noise of its images within the whole
            # batch (first_image), so the chunked batch is the whole one
            outs = [sbs.sample_distinct(h, part, n, 20, temperature, ((seed << 20) + batch_i, lo))
                    for lo, _, part in _chunks(feats, ensemble, len(image_ids), h.max_rows // n, whole=True)]
            ids, lens, phi, G = (torch.cat([o[k] for o in outs]).cpu().numpy() for k in (0, 1, 3, 4))
            for r in range(ids.shape[0]):                              # loader order: batch index, then image, then slot
                if lens[r] != 0:                                       # 0: an unoccupied slot (fewer than n sequences exist); its index stays taken
                    out.add(batch_i, r, image_ids[r // n], _pack_row(ids[r], phi[r], G[r]))
        pairs = out.gathered(lead.device)
    result = []
    for image_id, row in pairs:
        ids, score, pert = _unpack_row(row, True)
        result.append({"image_id": image_id, "caption": " ".join(_words(ids, lead.caption_vocab, True)), "score": score, "perturbed": pert})
    return result


def sample_distinct_ensemble_captions_json_generation(engines, dataloader, samples_per_image=5, temperature=1.0, seed=0, tqdm_visible=True, *,
                                                      weights=None):
    """Engine.sample_distinct_captions_json_generation for an ensemble of 1..4 engines (BUTD / AoA / NIC) of one vocabulary (an
    extension; include/icz.h: icz_ensemble_sample_distinct): `samples_per_image` distinct captions per image, a sample without
    replacement from the members' averaged word probabilities (`weights`: None = uniform) at the temperature.  Entries, seeding,
    sharding and gathering as the single-model method (the first engine's vocabulary); score = the ensemble's summed log-probability.
    Arguments are checked before any device work (ValueError)."""
    engines = _ensemble_engine_checks(engines, weights)
    return _sample_distinct_captions_json_generation(engines, weights, True, dataloader, samples_per_image, temperature, seed, tqdm_visible)


# ---- scoring given captions: what the Engine methods and the ensemble functions share ---------------------------------------------
def _check_score_entries(entries, captions_per_image):
    """the argument rules of score_captions_json that need neither an engine nor a device -> (entries as a list, n)"""
    from .scoring import MAX_WORDS, check_n
    n = check_n(captions_per_image)
    try:
        entries = list(entries)
    except TypeError:
        raise ValueError("entries must be a list of {'image_id', 'caption'} dicts") from None
    if len(entries) % n:
        raise ValueError("%d entries are not a multiple of %d captions per image" % (len(entries), n))
    for i, e in enumerate(entries):
        if not hasattr(e, "keys") or "image_id" not in e or not isinstance(e.get("caption"), str):
            raise ValueError("entry %d: expected a dict with 'image_id' and a 'caption' string" % i)
        if len(e["caption"].split()) > MAX_WORDS:
            raise ValueError("entry %d: caption with %d words: at most %d can be scored" % (i, len(e["caption"].split()), MAX_WORDS))
        if e["image_id"] != entries[i - i % n]["image_id"]:
            raise ValueError("entry %d: image_id %r inside the group of image %r" % (i, e["image_id"], entries[i - i % n]["image_id"]))
    return entries, n


def _score_chunks(h, feats, ensemble, ids, n):
    """ids [images x n, T] (numpy) of one loader batch under the handle and its features -> (logp [rows, T], score [rows]) as numpy
    arrays; scored in chunks of images where the rows exceed the handle's capacity"""
    from .scoring import score_captions
    refuse = "%d captions per image exceed the handle's row capacity %d" % (n, h.max_rows)
    logps, scores = [], []
    for lo, hi, part in _chunks(feats, ensemble, ids.shape[0] // n, h.max_rows // n, refuse):
        lp, sc = score_captions(h, part, ids[lo * n:hi * n], n)
        logps.append(lp.cpu().numpy())
        scores.append(sc.cpu().numpy())
    return np.concatenate(logps), np.concatenate(scores)


def _score_entries(engines, weights, dataloader, entries, n, tqdm_visible, ensemble=False):
    from .scoring import encode_captions, scored_lengths
    lead = engines[0]
    out, at = [], 0
    for _, image_ids, h, feats in _batches(engines, weights, ensemble, dataloader, "Scoring Process", tqdm_visible, shard=False):
        nb = len(image_ids)
        group = entries[at:at + nb * n]
        if len(group) != nb * n:
            raise ValueError("the loader holds more images than the %d entries cover" % len(entries))
        for j, image_id in enumerate(image_ids):
            if str(group[j * n]["image_id"]) != str(int(image_id) if not isinstance(image_id, str) else image_id):
                raise ValueError("entries %d..: image_id %r, but the loader's image is %r" % (at + j * n, group[j * n]["image_id"], image_id))
        ids = encode_captions([e["caption"] for e in group], lead.caption_vocab)
        logp, score = _score_chunks(h, feats, ensemble, ids, n)
        lens = scored_lengths(ids)
        for r, e in enumerate(group):
            d = dict(e)
            d["logprob"], d["tokens"], d["logprobs"] = float(score[r]), int(lens[r]), [float(x) for x in logp[r, :lens[r]]]
            out.append(d)
        at += nb * n
    if at != len(entries):
        raise ValueError("%d entries, but the loader's images cover %d" % (len(entries), at))
    return out


def _pick_by_likelihood(scored, n, lp):
    kind, alpha = lp
    out = []
    for i in range(0, len(scored), n):
        best, best_rank = None, None
        for e in scored[i:i + n]:
            t = e["tokens"]                      # >= 1: <end> is always scored
            rank = e["logprob"] / (t ** alpha if kind == 1 else ((5 + t) / 6.0) ** alpha if kind == 2 else 1.0)
            if best is None or rank > best_rank:
                best, best_rank = e, rank
        out.append({"image_id": best["image_id"], "caption": best["caption"], "logprob": best["logprob"], "rank_score": float(best_rank)})
    return out


def _reference_perplexity(eng, dataloader, tqdm_visible):
    from .scoring import MAX_CAPTIONS, encode_captions, scored_lengths
    eng.model.eval()
    total, tokens, captions = 0.0, 0, 0
    for img_ids, img_tensors, img_gts, supp_info_datas in _monitor(dataloader, "Scoring Process", tqdm_visible):
        refs = [list(img_gts[i]) for i in img_ids]
        most = max(len(r) for r in refs)
        for lo in range(0, most, MAX_CAPTIONS):
            n = min(MAX_CAPTIONS, most - lo)
            caps = [(r[lo:lo + n] + [None] * n)[:n] for r in refs]
            ids = encode_captions([c or "" for g in caps for c in g], eng.caption_vocab)
            for j, c in enumerate(c for g in caps for c in g):
                if c is None:
                    ids[j] = 0                   # no reference here: an empty caption, which scores nothing
            h, feats, _ = _prepare([eng], None, False, None, img_tensors, supp_info_datas)
            logp, _ = _score_chunks(h, feats, False, ids, n)
            lens = scored_lengths(ids)
            total += float(sum(np.sum(logp[r, :lens[r]], dtype=np.float64) for r in range(ids.shape[0])))
            tokens += int(lens.sum())
            captions += sum(c is not None for g in caps for c in g)
    if tokens == 0:
        raise ValueError("the loader holds no reference caption")
    nll = -total / tokens
    return {"ppl": float(np.exp(nll)), "nll_per_token": float(nll), "tokens": tokens, "captions": captions}


def score_ensemble_captions_json(engines, dataloader, entries, captions_per_image=1, tqdm_visible=True, *, weights=None):
    """Engine.score_captions_json for an ensemble of 1..4 engines (BUTD / AoA / NIC) of one vocabulary (an extension; include/icz.h:
    icz_ensemble_score_captions): every engine turns the shared batch into its own features, and each token's log-probability is
    that of the averaged word probabilities (`weights`: None = uniform).  Entries, result and errors as the single-model method
    (the first engine's vocabulary); arguments are checked before any device work (ValueError).  Not sharded: under
    torch.distributed every rank scores everything."""
    entries, n = _check_score_entries(entries, captions_per_image)
    engines = _ensemble_engine_checks(engines, weights)
    with _on_stream(engines[0]):
        return _score_entries(engines, weights, dataloader, entries, n, tqdm_visible, ensemble=True)


def rescore_ensemble_captions_json(engines, dataloader, entries, captions_per_image, length_penalty=None, tqdm_visible=True, *,
                                   weights=None):
    """Engine.rescore_captions_json under an ensemble: of every image the caption the ensemble finds most likely (length_penalty
    as there; ties: the first) -> one {"image_id", "caption", "logprob", "rank_score"} per image.  Not sharded: every rank scores
    everything."""
    lp = parse_length_penalty(length_penalty)
    entries, n = _check_score_entries(entries, captions_per_image)
    engines = _ensemble_engine_checks(engines, weights)
    with _on_stream(engines[0]):
        scored = _score_entries(engines, weights, dataloader, entries, n, tqdm_visible, ensemble=True)
    return _pick_by_likelihood(scored, n, lp)
