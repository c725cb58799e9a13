"""A poisoned allocator for tests: what `torch.empty` hands out holds a chosen byte instead of whatever the caching allocator
found (in a fresh process usually zeros, which hides every read of memory nobody wrote).

`poisoned(byte)` replaces `torch.empty` and `torch.empty_like` for the duration of a `with` block (streamflow_amd/ has no use of
`Tensor.new_empty`); every tensor they return has ALL bytes of its storage set to `byte`.  `torch.zeros` is left alone: a buffer
the project zeroes is under a contract, a buffer it does not zero is not.  While a stream capture is running nothing is filled,
so no memset node enters a graph.  Nesting is REFUSED (RuntimeError): two fills of one tensor would say nothing about which byte
a reader saw.  The originals are restored on the way out, also when the body raises.

The three bytes of the tests:
  0x00  zeros in every format -- the baseline, what a fresh process usually sees;
  0xFF  NaN as fp16 / fp32 / fp64, -1 as an integer;
  0x7B  finite and huge: 61280 as fp16, 1.3e36 as fp32, 6.5e286 as fp64 -- a read that fmax, a select or a comparison would hide
        from a NaN still changes the result.
(0x7E is not used: as fp16 0x7E7E is a NaN.)

`poison_plan(plan, byte)` overwrites, in place, every buffer of an existing engine plan that `_Plan.__init__` took from
`torch.empty` -- the "second clip on a used plan" case: everything the previous forward left behind is destroyed.  The k-octet
copies `ops.new_shadow` zeroed and the graph's staging inputs (`fmaps_in` / `cnets_in`) are not touched."""
import contextlib

import torch

BYTES = (0x00, 0xFF, 0x7B)

_active = []


def _capturing() -> bool:
    return bool(torch.cuda.is_available() and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing())


def fill_bytes(t: torch.Tensor, byte: int, empty=torch.empty) -> torch.Tensor:
    """Set every byte of t's storage to `byte` (t owns its storage: a fresh allocation, or a whole plan buffer)."""
    st = t.untyped_storage()
    if st.nbytes() > 0:
        empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(byte)
    return t


def fill_view(t: torch.Tensor, byte: int) -> torch.Tensor:
    """Set every byte of a contiguous tensor (which may be a slice of a larger allocation) to `byte`."""
    assert t.is_contiguous()
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned(byte: int):
    byte = int(byte)
    if not 0 <= byte <= 255:
        raise ValueError(f"poisoned: byte {byte} outside 0 .. 255")
    if _active:
        raise RuntimeError(f"poisoned({byte:#04x}) inside poisoned({_active[-1]:#04x}): nesting is refused")
    empty, empty_like = torch.empty, torch.empty_like

    def poisoned_empty(*args, **kw):
        t = empty(*args, **kw)
        return t if _capturing() else fill_bytes(t, byte, empty)

    def poisoned_empty_like(*args, **kw):
        t = empty_like(*args, **kw)
        return t if _capturing() else fill_bytes(t, byte, empty)

    _active.append(byte)
    torch.empty, torch.empty_like = poisoned_empty, poisoned_empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like
        _active.pop()


def plan_buffers(plan) -> list:
    """(name, tensor) of every buffer `_Plan.__init__` (streamflow_amd/engine.py) takes from torch.empty, in its order: the blocked
    volume or the row-major pyramid levels, the build's scratch, the fused GMA workspace and its stored weights, the attention
    matrix (fp32 and fp16), the workspace all activation planes are carved from, the upsampled flows."""
    out = []
    if plan.vol is not None:
        out.append(("vol", plan.vol.buf))
    for l, t in enumerate(plan.lvls or ()):
        out.append((f"lvls[{l}]", t))
    out.append(("corr_ws", plan.corr_ws))
    for name in ("flash_ws", "pbuf", "attn", "attn16"):
        if getattr(plan, name) is not None:
            out.append((name, getattr(plan, name)))
    out.append(("ws.buf", plan.ws.buf))
    out.append(("up", plan.up))
    return out


def poison_plan(plan, byte: int) -> None:
    assert not _capturing(), "poison_plan inside a stream capture"
    for _, t in plan_buffers(plan):
        fill_view(t, int(byte))
