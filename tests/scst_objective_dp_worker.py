"""Worker of tests/test_gpu_scst_objective.py: one of two data-parallel ranks on the SAME GPU (gloo backend).  Each rank takes three of
the six golden images and runs two samples_per_image = 4 SCST steps with the minimum-risk objective and an entropy bonus on them (its
share of the B K rows of explicit dropout masks / uniforms): the mask sum and the image count are all-reduced, and the parameters
must then equal those of one process on all six images (ICZ_TEST_REF)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as td

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import test_gpu_scst_multisample as tms  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    td.init_process_group(backend="gloo", rank=rank, world_size=world)
    from simpleimagecaptionzoo_amd import dist as icz_dist
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    K = 4
    g, fx, batches, _ = tms._steps(os.path.join(HERE, "golden"), K)
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    lo, hi = icz_dist.shard_range(B, rank, world)
    assert (lo, hi) == (3 * rank, 3 * rank + 3)
    eng = tms._engine(g, fx)
    eng.scst_terms = []
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for s, (ids, _, gts, supp) in enumerate(batches):
        rng = tms._rank_rng(B * K, lo * K, hi * K, 5 + s, R, E, A, H)      # every image's K rows stay on its rank
        batch = (ids[lo:hi], None, gts, supp[lo:hi])
        eng.SCST_objective_training_epoch([batch], opt, None, tqdm_visible=False, rngs=[rng], samples_per_image=K, objective="risk",
                                          entropy_weight=0.01)
    torch.cuda.synchronize()
    assert len(eng.scst_terms) == 2
    want = dict(np.load(os.environ["ICZ_TEST_REF"]))
    got = tms._params(eng)
    for k in want:
        # the per-rank prologue runs at another M: the tolerance of the existing two-rank tests (tests/test_gpu_engine.py _check_pinned)
        np.testing.assert_allclose(got[k], want[k], atol=5e-6, rtol=0, err_msg=k)
    td.barrier()
    td.destroy_process_group()
    print("rank %d ok" % rank)


main()
