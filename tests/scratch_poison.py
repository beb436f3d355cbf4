"""Poisoned memory for tests/test_gpu_scratch_poison.py, in its own process and in the child processes that the GPU modules start for
switches read once per process (tests/test_gpu_lists.py, tests/test_gpu_row_slots.py, test_long_n_lists).

fill_allocations   torch.empty and torch.empty_like hand out tensors whose bytes are one byte -> the function that undoes it
enter_child        first statement of such a child: nothing unless TRACS_TEST_POISON = "<byte>:<report file>" is in its environment
                   (the poison module's fixture puts it there); then the child switches the library's scratch poison on, fills its
                   allocations like the parent, and at exit appends one JSON line to the report file: its tag, the byte, and how often
                   it was handed each scratch slot -- what the parent's gate adds to its own counts."""
import atexit
import json
import os

ENV = "TRACS_TEST_POISON"


def fill_allocations(torch, byte):
    plain_empty, plain_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(byte)
        return t

    def empty(*args, **kw):
        t = plain_empty(*args, **kw)
        return t if kw.get("out") is not None else poisoned(t)

    def empty_like(*args, **kw):
        t = plain_like(*args, **kw)
        return poisoned(t) if t.is_contiguous() else t

    torch.empty, torch.empty_like = empty, empty_like

    def undo():
        torch.empty, torch.empty_like = plain_empty, plain_like
    return undo


def enter_child(tag):
    spec = os.environ.get(ENV)
    if not spec:
        return
    byte, path = spec.split(":", 1)
    byte = int(byte)
    import torch
    from tracs_amd import _lib, device
    fill_allocations(torch, byte)
    _lib.load().tracs_debug_poison_scratch(byte)
    device.scratch_hits()

    def report():
        with open(path, "a") as fh:
            fh.write(json.dumps({"tag": tag, "byte": byte, "hits": device.scratch_hits()}) + "\n")
    atexit.register(report)
