"""-m gpu: loops._on_stream, the context in which sieve_labels, components and object_table run torch's own operations on the raw stream
handle they are given.  The whole-map loops pass the net's stream, which is torch's default stream, handle 0 -- and torch makes a
stream from its POOL of an ExternalStream with a zero handle, unordered with stream 0: the sieve then cloned a map that the launches on
stream 0 had not written yet."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV   # noqa: E402


def test_on_stream_runs_torch_on_the_handle_it_is_given():
    from drs_amd import loops
    dev = torch.device(DEV)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    for handle in (None, 0):
        with loops._on_stream(dev, handle):
            assert torch.cuda.current_stream(dev).cuda_stream == 0
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != 0
    with loops._on_stream(dev, side.cuda_stream):
        assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
        with loops._on_stream(dev, 0):                     # back to the default stream from inside another stream's context
            assert torch.cuda.current_stream(dev).cuda_stream == 0
        with loops._on_stream(dev, side.cuda_stream):
            assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
    assert torch.cuda.current_stream(dev).cuda_stream == 0


def test_sieve_on_the_default_streams_handle_sees_what_that_stream_wrote():
    """the map is written by a long chain of launches on stream 0 right before the call, as validate_test does"""
    from drs_amd import loops
    h = w = 512
    for rep in range(3):
        src = torch.zeros(h * w, dtype=torch.uint8, device=DEV)
        big = torch.ones(1 << 26, dtype=torch.float32, device=DEV)
        for _ in range(8):
            big = big * 1.0001                              # work in front of the write on stream 0
        src += (big[:h * w] > 0).to(torch.uint8) * (1 + rep)
        out, info = loops.sieve_labels(src, h, w, 6, dict(min_size=4, connectivity=8), stream=0)
        assert bool((out == 1 + rep).all()) and info["changed_pixels"] == 0 and sum(info["objects_before"]) == 1
