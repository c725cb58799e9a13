"""The split route of sf_jpeg_decode_split (csrc/jpeg_sync_core.h, csrc/jpeg_decode.hip) restated in Python, from the header comment
of the entry point: unstuffing, the segments, the per-symbol step on a state (bit, slot, k) in its lenient and its strict form, the
rounds of a window, the block ordinals, the DC prefix sums and the status keys.  It shares no code with the C++ core and none with
jpeg_decode_cases.coefficients (whose coefficients it must reproduce): the Huffman decoder here is a 16-bit lookup on the unstuffed
stream held as one Python integer.  Also: the fixtures of tests/golden/jpeg_sync (four PIL files without DRI, made by
tests/golden/make_jpeg_sync_golden.py, for the window boundaries), Call with the two new arguments, and the helpers that compile
and run csrc/host/jpeg_sync_host_main.cpp under the host sanitizers.  Feeds tests/test_jpeg_sync_cases_cpu.py,
tests/test_jpeg_sync_host_cpu.py and tests/test_gpu_jpeg_sync.py."""
import functools
import os

import numpy as np

from tests import jpeg_cases as jc
from tests import jpeg_decode_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_sync")
WINDOW = 256                                    # kSyncWindow: segments whose chains are extended together
SEGMENT_BYTES = (8, 16, 128)
# (name, kind, h, w, channels, seed, PIL save options): no DRI; at 8-byte segments each has more segments than two windows hold
SYNC_CASES = [
    ("sync-444-96x128-q90", "waves", 96, 128, 3, 1, dict(quality=90, subsampling=0)),
    ("sync-420-96x128-q90", "waves", 96, 128, 3, 2, dict(quality=90, subsampling=2)),
    ("sync-grey-96x128-q90", "waves", 96, 128, 1, 3, dict(quality=90)),
    ("sync-444-48x64-q100-noise", "noise", 48, 64, 3, 4, dict(quality=100, subsampling=0)),
]
SYNC_NAMES = [c[0] for c in SYNC_CASES]
NAMES = dc.NAMES + SYNC_NAMES


def make(kind, h, w, channels, seed):
    """The images of SYNC_CASES: `waves` is two sine gratings plus a little noise (blocks of every length), `noise` is jc.make's."""
    if kind == "noise":
        return jc.make("noise", h, w, channels, seed)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 70 * np.sin((x * (3 + c) + y * (2 - c)) / 9.0 + seed) + 40 * np.sin(x * y / 300.0 + c) + rng.integers(-10, 11, size=(h, w))
              for c in range(3)]
    img = np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)
    return img if channels == 3 else img[:, :, 0].copy()


@functools.lru_cache(maxsize=None)
def load(name):
    if name in SYNC_NAMES:
        with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
            return f.read()
    return dc.load(name)


@functools.lru_cache(maxsize=None)
def expected():
    with np.load(os.path.join(GOLDEN, "expected.npz")) as z:
        out = {k: z[k] for k in z.files}
    out.update(dc.expected())
    return out


class Call(dc.Call):
    """dc.Call -- the arguments of one call for fixtures of one geometry -- plus segment_bytes and split_min_bytes; the names may be
    those of either fixture directory."""

    def __init__(self, names, segment_bytes=128, split_min_bytes=0):
        from streamflow_amd import jpeg_gpu
        self.names = list(names)
        blobs = [load(n) for n in self.names]
        parsed = [jpeg_gpu.parse(b, n) for b, n in zip(blobs, self.names)]
        assert len({p[:5] for p in parsed}) == 1, "one geometry per call"
        self.h, self.w, self.nc, self.hs, self.vs = parsed[0][:5]
        self.n = len(blobs)
        data, desc, tables = jpeg_gpu.pack(parsed, blobs)
        self.data, self.desc, self.tables = data.copy(), desc.copy(), tables.copy()
        self.segment_bytes, self.split_min_bytes = segment_bytes, split_min_bytes

    @classmethod
    def of(cls, call, segment_bytes=128, split_min_bytes=0):
        """A dc.Call (one of dc.mutations(), say) with the two arguments added."""
        c = object.__new__(cls)
        c.__dict__.update(call.__dict__)
        c.data, c.desc, c.tables = call.data.copy(), call.desc.copy(), call.tables.copy()
        c.segment_bytes, c.split_min_bytes = segment_bytes, split_min_bytes
        return c

    def copy(self):
        return Call.of(self, self.segment_bytes, self.split_min_bytes)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def unstuff(raw):
    """(stream, marker): raw without the 00 of every FF 00, up to the first FF that is the last byte or has another byte than 00
    behind it (marker: such an FF exists; running out of bits is then SF_JPEG_BAD_MARKER, not SF_JPEG_TRUNCATED)."""
    out, i = bytearray(), 0
    while i < len(raw):
        if raw[i] != 0xFF:
            out.append(raw[i])
            i += 1
        elif i + 1 < len(raw) and raw[i + 1] == 0:
            out.append(0xFF)
            i += 2
        else:
            return bytes(out), True
    return bytes(out), False


@functools.lru_cache(maxsize=None)
def _lut(bits, vals):
    """16-bit lookup of a Huffman specification: entry = length << 8 | symbol of the code the 16 bits start with, 0: none."""
    t, code, pos = np.zeros(1 << 16, np.int64), 0, 0
    for n, count in enumerate(bits, start=1):
        for sym in vals[pos:pos + count]:
            t[code << (16 - n):(code + 1) << (16 - n)] = n << 8 | sym
            code += 1
        pos += count
        code *= 2
    return t.tolist()


class Interval:
    """One interval's unstuffed stream with the tables and the geometry its walks need."""

    def __init__(self, raw, table_set, nc, hs, vs):
        self.u, self.marker = unstuff(bytes(raw))
        self.nbits = 8 * len(self.u)
        self.big = int.from_bytes(self.u + bytes(4), "big")
        self.luma = hs * vs
        self.bpm = self.luma + 2 if nc == 3 else 1
        rec = [bytes(table_set[608 * c:608 * (c + 1)]) for c in range(nc)]
        self.quant = [list(r[:64]) for r in rec]                            # natural order
        self.dc = [_lut(tuple(r[64:80]), tuple(r[80:336])) for r in rec]
        self.ac = [_lut(tuple(r[336:352]), tuple(r[352:608])) for r in rec]

    def comp(self, slot):
        return 0 if slot < self.luma else slot - self.luma + 1

    def failure(self):
        return dc.BAD_MARKER if self.marker else dc.TRUNCATED

    def peek(self, at, n):
        return (self.big >> (self.nbits + 32 - at - n)) & ((1 << n) - 1)

    def symbol(self, at, lut):
        """(status, symbol, at behind the code)."""
        left = self.nbits - at
        e = lut[self.peek(at, 16)]
        if e == 0:
            return (self.failure() if left < 16 else dc.BAD_CODE), 0, at
        if e >> 8 > left:
            return self.failure(), 0, at
        return dc.OK, e & 255, at + (e >> 8)

    def receive(self, at, s):
        if self.nbits - at < s:
            return None, at
        raw = self.peek(at, s)
        return (raw if raw >> (s - 1) else raw - (1 << s) + 1), at + s

    def step(self, at, c, k):
        """One symbol of a block of component c at zigzag index k (0: the DC symbol) -> (status, at, k, zi, v): k = 64 where the block
        is complete, zi >= 0 where the symbol carried the value v for zigzag index zi."""
        if k == 0:
            st, s, at = self.symbol(at, self.dc[c])
            if st:
                return st, at, k, -1, 0
            if s > 11:
                return dc.BAD_CATEGORY, at, k, -1, 0
            v = 0
            if s:
                v, at = self.receive(at, s)
                if v is None:
                    return self.failure(), at, k, -1, 0
            return dc.OK, at, 1, 0, v
        st, rs, at = self.symbol(at, self.ac[c])
        if st:
            return st, at, k, -1, 0
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 0:
                return dc.OK, at, 64, -1, 0
            if r != 15 or k + 16 > 63:
                return dc.BAD_RUN, at, k, -1, 0
            return dc.OK, at, k + 16, -1, 0
        if s > 10:
            return dc.BAD_CATEGORY, at, k, -1, 0
        if k + r > 63:
            return dc.BAD_RUN, at, k, -1, 0
        v, at = self.receive(at, s)
        if v is None:
            return self.failure(), at, k, -1, 0
        return dc.OK, at, k + r + 1, k + r, v

    def lenient(self, state, end_bit, lenient=True):
        """The walk that stores nothing: (exit state, blocks ended).  Any error ends the block one bit behind the failed symbol's
        first bit (lenient = False: the chain dies there instead, which is what the rule is for)."""
        at, slot, k = state
        blocks = 0
        while at < end_bit:
            st, nat, nk, _, _ = self.step(at, self.comp(slot), k)
            if st in (dc.TRUNCATED, dc.BAD_MARKER) or (st and not lenient):
                return (at, slot, k), blocks
            at, k = (at + 1, 64) if st else (nat, nk)
            if k == 64:
                k, slot, blocks = 0, (slot + 1) % self.bpm, blocks + 1
        return (at, slot, k), blocks

    def strict(self, state, end_bit, ordinal, total, last, put, errors):
        """The walk from a true entry: put(ordinal, slot, natural index, value) for every coefficient (AC dequantised, DC the raw
        difference) while ordinal < total; the first error ends it with its key in `errors`."""
        at, slot, k = state
        if ordinal >= total:
            return
        while at < end_bit:
            c = self.comp(slot)
            st, at, k, zi, v = self.step(at, c, k)
            if st == dc.OK and zi > 0:
                nat = int(jc.ZZ[zi])
                v *= self.quant[c][nat]
                if abs(v) > dc.COEF_MAX:
                    st = dc.COEF_RANGE
                else:
                    put(ordinal, slot, nat, v)
            elif st == dc.OK and zi == 0:
                put(ordinal, slot, 0, v)
            if st:
                errors.append((ordinal, 1, st))
                return
            if k == 64:
                k, slot, ordinal = 0, (slot + 1) % self.bpm, ordinal + 1
                if ordinal == total:
                    left = self.nbits - at
                    if self.marker:
                        errors.append((total, 0, dc.BAD_MARKER))
                    elif left > 7 or (left and self.peek(at, left) != (1 << left) - 1):
                        errors.append((total, 0, dc.NOT_CONSUMED))
                    return
        if last:
            errors.append((ordinal, 1, self.failure()))

    def segments(self, S):
        return max(1, -(-len(self.u) // S))

    def end_bit(self, s, S):
        return 8 * min((s + 1) * S, len(self.u))

    def synchronise(self, S, lenient=True):
        """(entry states, block ordinals, rounds, re-decodes): the speculative walk of every segment from (its first bit, 0, 0), then
        per window of WINDOW segments Jacobi rounds -- segment k's entry becomes segment k - 1's exit of the round before, the
        window's first takes the previous window's final exit, the interval's first (0, 0, 0); only changed entries walk again --
        until a round changes nothing."""
        n = self.segments(S)
        entry = [(8 * s * S, 0, 0) for s in range(n)]
        walked = [self.lenient(entry[s], self.end_bit(s, S), lenient) for s in range(n)]
        carry, rounds, redecodes = (0, 0, 0), 0, 0
        for w0 in range(0, n, WINDOW):
            w1 = min(w0 + WINDOW, n)
            while True:
                new = [carry] + [walked[s][0] for s in range(w0, w1 - 1)]
                changed = [s for s in range(w0, w1) if new[s - w0] != entry[s]]
                if not changed:
                    break
                rounds, redecodes = rounds + 1, redecodes + len(changed)
                assert rounds <= n + 1
                for s in changed:
                    entry[s] = new[s - w0]
                    walked[s] = self.lenient(entry[s], self.end_bit(s, S), lenient)
            carry = walked[w1 - 1][0]
        ordinals = np.concatenate([[0], np.cumsum([b for _, b in walked])])[:n]
        return entry, [int(o) for o in ordinals], rounds, redecodes

    def serial_entries(self, S):
        """The entry state of every segment from ONE lenient walk over the whole stream: the first symbol boundary at or behind the
        segment's first bit (or where the walk got stuck in front of it)."""
        out, state = [(0, 0, 0)], (0, 0, 0)
        for s in range(1, self.segments(S)):
            state, _ = self.lenient(state, 8 * s * S)
            out.append(state)
        return out


def decode_interval(iv, S, n_mcus, put):
    """The split route on one interval -> (status, rounds, re-decodes, segments, entries).  put(ordinal, slot, nat, v) receives the
    coefficients; the DC stage works on what put() stored, through get_dc / set_dc of the caller (see decode)."""
    entry, ordinals, rounds, redecodes = iv.synchronise(S)
    total, errors, n = n_mcus * iv.bpm, [], iv.segments(S)
    for s in range(n):
        iv.strict(entry[s], iv.end_bit(s, S), ordinals[s], total, s == n - 1, put, errors)
    return errors, rounds, redecodes, n, entry


def decode(call):
    """The entropy stage of sf_jpeg_decode_split on a Call -> dict(status int32 [n], interval_status, rounds, redecodes, segments (per
    interval; rounds -1: not split), coef int16 [n, blocks, 64] in the device's layout, entries {interval: states}).  An interval
    below split_min_bytes is walked as ONE segment -- the coefficients and whether its status is zero are those of the wave route,
    which tests/jpeg_decode_cases.py restates; a nonzero word is the split route's."""
    hs, vs, nc = call.hs, call.vs, call.nc
    mcux, mcuy = -(-call.w // (8 * hs)), -(-call.h // (8 * vs))
    mcus, blocks = mcux * mcuy, call.image_blocks()
    bw = [mcux * hs] + [mcux] * (nc - 1)
    comp_off = np.concatenate([[0], np.cumsum([mcux * hs * mcuy * vs] + [mcus] * (nc - 1))])
    coef = np.zeros((call.n, blocks, 64), np.int64)
    res = dict(interval_status=[], rounds=[], redecodes=[], segments=[], entries={})
    first_error, covered = {}, np.zeros(call.n, np.int64)
    for i, d in enumerate(call.desc):
        in_off, in_len, image, first, n, tset = (int(v) for v in d)
        ok = 0 <= in_off <= len(call.data) and 0 <= in_len <= len(call.data) - in_off and 0 <= image < call.n and first >= 0 and \
            n >= 1 and first <= mcus and n <= mcus - first and 0 <= tset < len(call.tables)
        rounds = redecodes = segs = 0
        if not ok:
            st, rounds = dc.BAD_DESC, -1
        elif not _tables_ok(call.tables[tset], nc):
            st, rounds = dc.BAD_TABLE, -1
        else:
            iv = Interval(call.data[in_off:in_off + in_len].tobytes(), call.tables[tset].tobytes(), nc, hs, vs)

            def index(ordinal, slot):
                mi = first + ordinal // iv.bpm
                c = iv.comp(slot)
                j = slot if c == 0 else 0
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                my, mx = divmod(mi, mcux)
                return c, int(comp_off[c]) + (my * cv + j // ch) * bw[c] + mx * ch + j % ch

            def put(ordinal, slot, nat, v):
                coef[image, index(ordinal, slot)[1], nat] = v

            split = in_len >= call.split_min_bytes
            S = call.segment_bytes if split else max(8, 1 << max(in_len, 1).bit_length())
            errors, rounds, redecodes, segs, entry = decode_interval(iv, S, n, put)
            if split:
                res["entries"][i] = entry
            else:
                rounds = -1
            pred = [0] * nc                                                 # the DC stage: prefix sums in scan order, 64 bits and more
            for ordinal in range(n * iv.bpm):
                slot = ordinal % iv.bpm
                c, b = index(ordinal, slot)
                pred[c] += int(coef[image, b, 0])
                v = pred[c] * iv.quant[c][0]
                if abs(pred[c]) > dc.COEF_MAX or abs(v) > dc.COEF_MAX:
                    errors.append((ordinal, 0, dc.COEF_RANGE))
                    v = 0
                coef[image, b, 0] = v
                if int(np.abs(coef[image, b]).sum()) > dc.BLOCK_SUM_MAX:
                    errors.append((ordinal, 2, dc.COEF_RANGE))
            st = min(errors)[2] if errors else dc.OK                        # the smallest key: the first error in stream order
        res["interval_status"].append(st)
        res["rounds"].append(rounds), res["redecodes"].append(redecodes), res["segments"].append(segs)
        at = min(max(image, 0), call.n - 1)
        if st:
            first_error.setdefault(at, st)
        else:
            covered[at] += n
    res["status"] = np.array([first_error.get(i, dc.OK if covered[i] == mcus else dc.BAD_DESC) for i in range(call.n)], np.int32)
    res["coef"] = coef.astype(np.int16)
    return res


def _tables_ok(table_set, nc):
    for c in range(nc):
        for off in (64, 336):
            bits = [int(b) for b in table_set[608 * c + off:608 * c + off + 16]]
            code = 0
            for n, count in enumerate(bits, start=1):
                code += count
                if count and code > 1 << n:
                    return False
                code *= 2
            if sum(bits) > 256:
                return False
    return True


# ---- the sanitized host program ---------------------------------------------------------------------------------------------------------
def host_program(directory):
    """csrc/host/jpeg_sync_host_main.cpp compiled with the host sanitizers -> the program's path (as dc.host_program does)."""
    import shutil
    import subprocess
    from streamflow_amd import build
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(repo, "streamflow_amd", "csrc", "host", "jpeg_sync_host_main.cpp")
    cands = [os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin", "clang++"),
             "/opt/rocm/lib/llvm/bin/clang++"]
    cc = next((c for c in cands if os.path.exists(c)), None) or shutil.which("clang++")
    assert cc, "the ROCm clang++ is needed to build the host program"
    exe = os.path.join(str(directory), "jpeg_sync_host")
    r = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", src,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host(exe, calls, directory, tag):
    """[Call] -> [dict(status, interval_status, rounds, redecodes, segments, coef int16 [n, blocks, 64])]; the run must be clean: exit
    code 0, no sanitizer report."""
    import struct
    import subprocess
    fin, fout = os.path.join(str(directory), f"{tag}.in"), os.path.join(str(directory), f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(calls)))
        for c in calls:
            f.write(struct.pack("<8iqiq", c.h, c.w, c.nc, c.hs, c.vs, c.n, len(c.desc), len(c.tables), len(c.data), c.segment_bytes,
                                c.split_min_bytes))
            f.write(c.data.tobytes() + np.ascontiguousarray(c.desc, np.int64).tobytes() + np.ascontiguousarray(c.tables, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    res, at, out = np.fromfile(fout, np.uint8), 0, []

    def words(count):
        nonlocal at
        v = res[at:at + 4 * count].view(np.int32).copy()
        at += 4 * count
        return v

    for c in calls:
        ncoef, k = c.n * c.image_blocks() * 64, len(c.desc)
        one = dict(status=words(c.n), interval_status=words(k), rounds=words(k), redecodes=words(k), segments=words(k))
        one["coef"] = res[at:at + 2 * ncoef].view(np.int16).reshape(c.n, -1, 64).copy()
        at += 2 * ncoef
        out.append(one)
    assert at == len(res)
    return out
