"""The hipGraph capture recipe, once: warm the step up on a side stream, then capture it on static buffers.

Every buffer the step reads or writes must be allocated by the caller and outlive the graph, and a warm-up that must
not move state (parameters, track state) is the caller's to undo between the two halves.
"""
import torch


def warm_up(step, n=1):
    """Run step() max(1, n) times on a side stream, fenced against the current stream on both sides."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, n)):
            step()
    torch.cuda.current_stream().wait_stream(side)


def capture(step, pool=None):
    """Capture step() -> (graph, what step() returned: the graph's static outputs).  pool: another graph's pool()."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool):
        out = step()
    return graph, out


def warm_capture(step, warmup=1, pool=None):
    warm_up(step, warmup)
    return capture(step, pool)
