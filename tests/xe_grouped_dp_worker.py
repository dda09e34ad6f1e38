"""Worker of tests/test_gpu_xe_grouped.py: one of two data-parallel ranks on the SAME GPU (gloo backend).  Each rank takes three of the
six golden images and runs two training_epoch_grouped steps on them: the dropout masks are the same for every row, the token count is
all-reduced, the gradients are summed, and the parameters must then equal those of one process on all six images (ICZ_TEST_REF)."""
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
import test_gpu_xe_grouped as txg  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    td.init_process_group(backend="gloo", rank=rank, world_size=world)
    from simpleimagecaptionzoo_amd import dist as icz_dist
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, _ = tms._steps(os.path.join(HERE, "golden"), 1)
    B = int(g["dims"][0])
    lo, hi = icz_dist.shard_range(B, rank, world)
    assert (lo, hi) == (3 * rank, 3 * rank + 3)
    eng = tms._engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    crit = type("Crit", (), {"smoothing": 0.1})()
    for s, (ids, _, gts, supp) in enumerate(batches):
        rng = txg.engine_rng((hi - lo) * txg.DP_K, 60 + s, g)
        losses = eng.training_epoch_grouped([(ids[lo:hi], None, gts, supp[lo:hi])], opt, crit, tqdm_visible=False, rngs=[rng],
                                            captions_per_image=txg.DP_K)
        assert len(losses) == 1 and np.isfinite(losses[0].item())
    torch.cuda.synchronize()
    want = dict(np.load(os.environ["ICZ_TEST_REF"]))
    got = tms._params(eng)
    for k in want:
        # the per-rank prologue runs at another M: the tolerance of the existing two-rank tests (tests/test_gpu_engine.py _check_pinned)
        np.testing.assert_allclose(got[k], want[k], atol=5e-6, rtol=0, err_msg=k)
    td.barrier()
    td.destroy_process_group()
    print("rank %d ok" % rank)


main()
