"""hip_ops.graph_capture keeps Python's cyclic garbage collector off while a stream capture is open: a collection that starts
inside a capture (in whichever thread allocates next) would destroy dead cycles there -- earlier pipelines' hipGraphs among them."""
import gc

import pytest
import torch

from stratanet2_vegetation_coverage_maps_amd import hip_ops as ops

pytestmark = pytest.mark.gpu


def test_collector_is_off_inside_a_capture_and_restored_after():
    x = torch.zeros(16, device="cuda:0")
    side = ops.shared_stream("cuda:0", "capture")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x += 1                                           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert gc.isenabled()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph, "cuda:0"):
        inside = gc.isenabled()
        x += 1
    assert inside is False and gc.isenabled()
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [2.0] * 16
    # a block that raises, and a caller who had the collector off already
    with pytest.raises(RuntimeError, match="stop"):
        with ops.graph_capture(torch.cuda.CUDAGraph(), "cuda:0"):
            x += 1
            raise RuntimeError("stop")
    assert gc.isenabled()
    gc.disable()
    try:
        with ops.graph_capture(torch.cuda.CUDAGraph(), "cuda:0"):
            x += 1
        assert not gc.isenabled()
    finally:
        gc.enable()
    torch.cuda.synchronize()
