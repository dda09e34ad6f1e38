"""Worker of tests/test_gpu_aoa_refiner_train.py::test_two_ranks_reproduce_one_process: one of WORLD_SIZE data-parallel ranks on the
SAME GPU (gloo, as tests/dp_worker.py).  Every rank first runs two XE steps and one SCST step of AoADetection_Eng(train_refiner=True)
on the whole batch in this process (no process group yet: the single-process reference), then joins the group and repeats them on
its share of the batch; every parameter -- the refiner's and the projection's too -- must end where the reference ended."""
import os
import sys

import numpy as np
import torch
import torch.distributed as td

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import _aoa_refiner as ar  # noqa: E402

CFG = (4, 5, 24, 32, 16, 31, 4, 20, None, None)       # B, R, D, Hd, E, V, NH, T
LENGTHS = [5, 4, 2, 2]
AXIS = {"proj": 0}                                     # the batch axis of a mask (1 for the per-layer / per-step ones)


class _Crit:
    smoothing = 0.1


def _supp(feats):
    return tuple({"bu_feat": feats[i], "bu_bbox": np.zeros((feats.shape[1], 4), np.float32)} for i in range(feats.shape[0]))


def run(lo, hi):
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, init_optimizer
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    B, R, D, Hd, E, V, NH = CFG[:7]
    vocab = synthetic_vocab(V)
    gts = synthetic_references(B, [vocab.ix2word[i] for i in range(V)], seed=5)
    eng = AoADetection_Eng({"model_type": "AoADetection", "embed_dim": E, "hidden_dim": Hd, "num_heads": NH, "num_regions": R, "enc_dim": D},
                           "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=document_frequency(gts), max_batch=8,
                           train_refiner=True)
    eng.model.load_state_dict(ar.state_dict_of(CFG, 400), strict=True)

    def rng_of(seed, T, with_u):
        masks, u = ar.masks_of(CFG, seed, B, T)
        cut = {k: np.ascontiguousarray(np.take(v, range(lo, hi), axis=AXIS.get(k, 1))) for k, v in masks.items()}
        return ar.device_rng(cut, np.ascontiguousarray(u[:, lo:hi]) if with_u else None)

    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 4e-4}), 4e-4)
    for s in range(2):
        feats = ar.feats_of(CFG, 410 + s).numpy()[lo:hi]
        caps = ar.captions_of(CFG, LENGTHS, 420 + s)[lo:hi]
        batch = (tuple(range(lo, hi)), None, caps, [n + 1 for n in LENGTHS[lo:hi]], _supp(feats))
        eng.training_epoch([batch], opt, _Crit(), tqdm_visible=False, rngs=[rng_of(430 + s, max(LENGTHS), False)])
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    feats = ar.feats_of(CFG, 412).numpy()[lo:hi]
    eng.SCST_training_epoch([(tuple(range(lo, hi)), None, gts, _supp(feats))], opt, None, tqdm_visible=False, rngs=[rng_of(432, 20, True)])
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    B = CFG[0]
    want = run(0, B)
    td.init_process_group(backend="gloo", rank=rank, world_size=world)
    from simpleimagecaptionzoo_amd import dist as icz_dist
    lo, hi = icz_dist.shard_range(B, rank, world)
    assert icz_dist.is_distributed() and hi > lo
    got = run(lo, hi)
    sd0 = ar.state_dict_of(CFG, 400)
    moved = 0
    for k, v in got.items():
        # three Adam steps; a zero-gradient tensor (every linear_K.bias) moves by rounding noise, at most lr per step
        tol = (2 * 4e-4 + 2e-5) * 1.01 if k.endswith("linear_K.bias") else 3 * 5e-6
        np.testing.assert_allclose(v.numpy(), want[k].numpy(), atol=tol, rtol=0, err_msg=k)
        moved += int(not k.startswith("decoder.") and not torch.equal(v, sd0[k]))
    assert moved == 64, moved
    td.barrier()
    td.destroy_process_group()
    print("rank %d ok" % rank)


main()
