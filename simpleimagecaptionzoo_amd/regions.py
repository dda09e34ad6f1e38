"""Region sets of a batch, shared by the region-attending handles (BUTD, AoA): `'fixed'` (36 boxes, `bu_masks` None), the
7x7 grid (49) and `'adaptive'` (10..100 boxes per image, padded to the batch's largest count with prefix `bu_masks`,
BUTD_Engine.py:35-46 / AoA_Engine.py:33-46).  A handle is created for the largest region count it will see and every batch may
be narrower; a RegionBatch carries the valid count of each image beside the padded tensor."""
import collections
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr

# features [B, R, D] + the valid region count of each image (host ints; None = all R valid)
RegionBatch = collections.namedtuple("RegionBatch", "feats counts")


def counts_from_masks(bu_masks):
    """bu_masks [B, R] (1 = valid) -> per-image counts.  The reference builds prefix masks (AoA_Engine.py:37-40) and itself
    reads them as lengths (pack_wrapper, AoA_Model.py:652); anything else is rejected."""
    m = bu_masks.detach()
    counts = m.long().sum(1)
    prefix = torch.arange(m.shape[1], device=m.device).unsqueeze(0) < counts.unsqueeze(1)
    if not bool(((m != 0) == prefix).all()):
        raise ValueError("bu_masks must mark a leading run of valid regions per image (AoA_Engine.py:37-40)")
    return counts.tolist()


def region_features(visual_inputs):
    """What a mask-aware Captioner hands its handle: bu_feats, as a RegionBatch where the batch carries `bu_masks` (the counts
    are `bu_counts` when the Engine supplies them, else read back from the mask)."""
    feats = visual_inputs["bu_feats"].detach()
    masks = visual_inputs.get("bu_masks")
    if masks is None:
        return feats
    counts = visual_inputs.get("bu_counts")
    return RegionBatch(feats, list(counts) if counts is not None else counts_from_masks(masks))


class RegionSets:
    """Mixed into a DecoderHandle whose library has icz_<family>_set_regions (listed in its `_own_entries`): the handle's R is a
    capacity, `_feats` takes a tensor (B, 1..R, D) or a RegionBatch and sets the layout of the calls that follow.  Everything here is
    plumbing behind `_feats` (no public method: AoaHandle publishes its own set_regions on top)."""

    def _regions_init(self):
        self._regions = (self.R, None)
        self._counts_dev = None

    @property
    def regions(self):
        """Regions per image (the row stride) of the current batch layout."""
        return self._regions[0]

    def _set_regions(self, regions, counts=None):
        """icz_<family>_set_regions: the batches that follow are [B, regions, D]; counts = valid regions per image or None."""
        if counts is None:
            if self._regions != (regions, None):
                check(self._e.set_regions(self._h, int(regions), None, None, 0))
                self._regions, self._counts_dev = (regions, None), None
            return
        counts = [int(c) for c in counts]
        host = (C.c_int32 * len(counts))(*counts)
        dev = torch.tensor(counts, dtype=torch.int32, device=self.device)
        check(self._e.set_regions(self._h, int(regions), ptr(dev), host, len(counts)))
        # the kernels of the following calls read `dev`: it stays referenced until the next set_regions, and torch's
        # caching allocator hands its memory out again only in stream order
        self._regions, self._counts_dev = (regions, tuple(counts)), dev

    def _feats(self, f):
        counts = None
        if isinstance(f, RegionBatch):
            f, counts = f
        if f.dtype != torch.float32 or not f.is_cuda or f.dim() != 3 or f.shape[2] != self.D or not 1 <= f.shape[1] <= self.R:
            raise _lib.IczError("bu_feats must be an fp32 CUDA tensor (B, 1..%d, %d)" % (self.R, self.D))
        if counts is not None and len(counts) != f.shape[0]:
            raise _lib.IczError("%d region counts for %d images" % (len(counts), f.shape[0]))
        self._set_regions(f.shape[1], counts)
        return f.contiguous()
