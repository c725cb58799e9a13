"""Guard-banded device buffers for the descriptor tests (tests/test_gpu_gemm_descriptors.py, tests/test_gpu_chain_descriptors.py):
a logical [batch][rows][cols] view placed inside a larger flat allocation -- leading dimension beyond the extent, a gap between
images, a base off the allocation's start -- whose every other element holds a known fill (NaN for operands: a read that reaches a
result shows; a finite sentinel for outputs) and must come back bitwise unchanged.  GuardedBytes: a byte workspace of exactly the
size an entry point asks for, between two guard bands (tests/test_gpu_attn_kernels.py)."""
import numpy as np
import torch

SENTINEL = 1234.5


class Guarded:
    """A [batch][rows][cols] view inside a flat buffer filled with `fill`; image z starts at off + z * stride.
    Row mode (fp32 planes, fp16 rows): element (r, c) at row_off(r) + c, row_off(r) = r * ld, or in groups of `group` rows
    `group_stride` apart.
    k-octet mode (koct=True: SF_LAYOUT_F16_KOCT with a leading dimension): element (r, c) at ((r / 8) * ld + c) * 8 + r % 8, the rows
    of a group counted from the group's start.  `rows` need not be a multiple of 8: the rows past it in the last octet are outside
    the view.
    The buffer ends `tail` elements after the last image's stride, so no descriptor built from the view can span past it."""

    def __init__(self, dev, batch, rows, cols, off, ld, stride, fill, dtype=torch.float32, group=0, group_stride=0, koct=False,
                 tail=0):
        assert ld >= cols and off >= 0 and (not group or rows % group == 0 or not koct)

        def elem(r, c):
            rl = r % group if group else r
            goff = (r // group) * group_stride if group else 0
            return goff + (((rl // 8) * ld + c) * 8 + rl % 8 if koct else rl * ld + c)

        assert stride >= elem(rows - 1, cols - 1) + 1
        self.off, self.ld, self.stride, self.dtype, self.group_stride, self.fill = off, ld, stride, dtype, group_stride, fill
        self.buf = torch.full((off + batch * stride + tail,), fill, dtype=dtype, device=dev)
        z = np.arange(batch)[:, None, None]
        r = np.arange(rows)[None, :, None]
        c = np.arange(cols)[None, None, :]
        self.idx = torch.from_numpy((off + z * stride + elem(r, c)).reshape(-1)).to(dev)
        self.shape = (batch, rows, cols)
        self.inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        self.inside[self.idx] = True

    def put(self, t):
        self.buf[self.idx] = t.to(device=self.buf.device, dtype=self.dtype).reshape(-1)
        self.snap = self.buf.clone()
        return self

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * self.off

    def region(self):
        return self.buf[self.idx].view(self.shape)

    def outside_unchanged(self, before=None):
        """Every element outside the view is bitwise what it was (the fill, or the snapshot taken by put())."""
        ref = getattr(self, "snap", None) if before is None else before
        if ref is None:
            ref = torch.full_like(self.buf, self.fill)
        a, b = self.buf[~self.inside], ref[~self.inside]
        return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


class Placed(Guarded):
    """A Guarded view at an EXPLICIT placement (tests/gemm_packed_cases.py place(): off, ld, stride, group_stride in elements), for
    the k-octet forms in particular: a base 16 bytes into the allocation, ld > cols, a gap of a multiple of 8 halves after every
    image, groups of rows with a gap between them.  kind: 'f32' fp32 planes, 'h16' fp16 rows, 'koct' fp16 k-octet planes.
    k-octet views whose rows are no multiple of 8 have a TAIL: the rows past `rows` in the last octet.  They are outside the view,
    but a consumer may read them (they meet zero weights and must be finite) and a c_f16 = 2 producer may write them: `tail_fill`
    puts a finite value there, tail() returns them and outside_unchanged(tail_free=True) leaves them out of the comparison."""

    def __init__(self, dev, kind, batch, rows, cols, off, ld, stride, group, group_stride, fill, tail_fill=None):
        koct = kind == "koct"
        super().__init__(dev, batch, rows, cols, off, ld, stride, fill, torch.float32 if kind == "f32" else torch.float16,
                         group=group, group_stride=group_stride, koct=koct, tail=8)
        self.kind = kind
        self.tail_idx = None
        if koct and rows % 8:
            rl = (rows - 1) % group if group else rows - 1                  # last row, counted inside its group
            goff = ((rows - 1) // group) * group_stride if group else 0
            z = np.arange(batch)[:, None, None]
            r = np.arange(rl % 8 + 1, 8)[None, :, None]
            c = np.arange(cols)[None, None, :]
            self.tail_idx = torch.from_numpy((off + z * stride + goff + ((rl // 8) * ld + c) * 8 + r).reshape(-1)).to(dev)
            if tail_fill is not None:
                self.buf[self.tail_idx] = tail_fill
        self.snap = self.buf.clone()

    def tail(self):
        return self.buf[self.tail_idx].float()

    def outside_unchanged(self, before=None, tail_free=False):
        ref = self.snap if before is None else before
        keep = ~self.inside
        if tail_free and self.tail_idx is not None:
            keep[self.tail_idx] = False
        return bool(torch.equal(_bits(self.buf[keep]), _bits(ref[keep])))

    def untouched(self):
        """The whole allocation, view included, is bitwise what put() left (operands)."""
        return bool(torch.equal(_bits(self.buf), _bits(self.snap)))


class GuardedBytes:
    """A byte workspace of exactly `size` bytes between two guard bands of `guard` bytes (a multiple of `align`, so the workspace keeps
    the allocation's alignment; shift > 0 moves it off that alignment).  The workspace is filled with `fill`, the bands with `band`;
    guards_unchanged(): both bands are bitwise what they were."""

    def __init__(self, dev, size, fill=0x7F, band=0xA5, guard=4096, shift=0):
        self.size, self.guard, self.band = int(size), guard + shift, band
        self.buf = torch.full((self.guard + self.size + guard,), band, dtype=torch.uint8, device=dev)
        self.view().fill_(fill)

    def view(self):
        return self.buf[self.guard: self.guard + self.size]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.guard

    def guards_unchanged(self):
        return bool((self.buf[: self.guard] == self.band).all()) and bool((self.buf[self.guard + self.size:] == self.band).all())


def _operand(dev, rng, t, unaligned, dtype=torch.float32):
    """Place logical [batch][rows][cols] data t in a NaN-poisoned allocation: ld padding, 1-3 extra rows after each image,
    base 0 or (unaligned) 1-3 floats off 16 bytes (2-6 halves for fp16: a stored-fp16 B needs 4-byte alignment)."""
    batch, rows, cols = t.shape
    q = 8 if dtype == torch.float16 else 4                      # elements per 16 bytes
    if unaligned:
        off = int(rng.choice([2, 4, 6])) if dtype == torch.float16 else int(rng.integers(1, 4))
        ld = cols + (cols % 2 + int(rng.choice([0, 2, 4])) if dtype == torch.float16 else int(rng.integers(1, 6)))   # even
    else:
        off, ld = q * int(rng.integers(0, 2)), -(-cols // q) * q + q * int(rng.integers(0, 3))
    stride = (rows + int(rng.integers(1, 4))) * ld
    stride = -(-stride // q) * q if not unaligned else stride + int(rng.integers(0, 3))
    return Guarded(dev, batch, rows, cols, off, ld, stride, float("nan"), dtype).put(t)


def _output(dev, rng, batch, rows, cols, unaligned, fill=SENTINEL, group=0):
    """Output / residual placement: ld > cols, image stride > rows * ld (+ a gap between row groups for a grouped view)."""
    if unaligned:
        off, ld = int(rng.integers(1, 4)), cols + int(rng.integers(1, 6))
    else:
        off, ld = 4 * int(rng.integers(0, 2)), -(-(cols + 1) // 4) * 4 + 4 * int(rng.integers(0, 2))
    gs = 0
    if group:
        gs = group * ld + 4 * int(rng.integers(1, 4))
        span = ((rows - 1) // group) * gs + ((rows - 1) % group) * ld + cols
    else:
        span = rows * ld
    stride = span + 4 * int(rng.integers(1, 4))
    return Guarded(dev, batch, rows, cols, off, ld, stride, fill, group=group, group_stride=gs)
