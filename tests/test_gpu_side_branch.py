"""The fork / join rule of the decoders' side streams (SideStream::Branch, csrc/decoder_core.h) on its own, through the test entry
icz_test_side_branch (include/icz.h): a two-kernel captured graph with one branch, made to fail at each point of the branch's life.
An error inside a forked capture must surface as itself -- its own status and text, not a capture failure -- and leave the stream
usable.  Host error returns only; every case takes milliseconds."""
import pytest
import torch

from simpleimagecaptionzoo_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
WRITTEN = [1.0, 2.0]              # out2[0] from the caller's stream, out2[1] from the branch's


def _run(fail_at, inline, out, stream):
    return lib().icz_test_side_branch(fail_at, inline, ptr(out), stream.cuda_stream)


@pytest.mark.parametrize("inline", [0, 1])
@pytest.mark.parametrize("fail_at", [0, 1, 2, 3])
def test_error_inside_a_forked_capture_surfaces_as_itself(fail_at, inline):
    stream = torch.cuda.Stream()
    out = torch.zeros(2, device="cuda")
    torch.cuda.synchronize()
    assert _run(fail_at, inline, out, stream) == ERR_INVALID
    msg = lib().icz_last_error().decode()
    assert msg == "side-branch test: stage %d" % fail_at
    assert "hipStreamEndCapture" not in msg
    # the stream is not left capturing: the same stream takes the whole graph next
    assert _run(-1, inline, out, stream) == 0, lib().icz_last_error().decode()
    stream.synchronize()
    assert out.tolist() == WRITTEN


@pytest.mark.parametrize("inline", [0, 1])
def test_second_call_replays_the_graph(inline):
    stream = torch.cuda.Stream()
    out = torch.zeros(2, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):                # the first call captures (or finds the graph of an earlier test: the key is the buffer), the second replays
        assert _run(-1, inline, out, stream) == 0, lib().icz_last_error().decode()
        stream.synchronize()
        assert out.tolist() == WRITTEN
        out.zero_()
        torch.cuda.synchronize()
