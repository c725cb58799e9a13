"""CPU: the restatement the split route of the GPU JPEG decoder is held to (tests/jpeg_sync_cases.py) against the serial restatement
(tests/jpeg_decode_cases.coefficients, itself pinned to PIL), on the 70 files of tests/golden/jpeg_decode and the four of
tests/golden/jpeg_sync, every interval split, at segments of 8, 16 and 128 bytes.  Every comparison is bitwise.  Also what the
method rests on: the fixed point of the rounds is the serial walk's states, the rounds stay at or below the segment count, the
slow-synchronisation case really is slow, and without the lenient rule the chains die."""
import os

import numpy as np
import pytest

from tests import jpeg_decode_cases as dc
from tests import jpeg_sync_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interval(name, row=0):
    c = sc.Call([name])
    off, length, _, _, _, tset = (int(v) for v in c.desc[row])
    return sc.Interval(c.data[off:off + length].tobytes(), c.tables[tset].tobytes(), c.nc, c.hs, c.vs)


def test_the_new_fixtures_are_pil_files_without_dri_that_span_more_than_two_windows():
    total = os.path.getsize(os.path.join(sc.GOLDEN, "expected.npz"))
    for name, _, h, w, _, _, _ in sc.SYNC_CASES:
        blob = sc.load(name)
        info = dc.walk(blob)
        total += len(blob)
        assert info["restart"] == 0 and len(info["intervals"]) == 1 and (info["h"], info["w"]) == (h, w) and h <= 96 and w <= 128
        assert interval(name).segments(8) > 2 * sc.WINDOW
        assert np.array_equal(dc.decode_ref(blob), sc.expected()[name]), name           # the serial restatement == PIL's recorded pixels
    assert total < 150 * 1024
    assert sorted(os.listdir(sc.GOLDEN)) == sorted([n + ".jpg" for n in sc.SYNC_NAMES] + ["expected.npz"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_coefficients_states_and_rounds(name):
    """Per segment size: the split route's coefficients are the serial decoder's; the entry states the rounds end at are those of
    one serial walk; the rounds of all windows together stay at or below the segment count."""
    info, want = dc.coefficients(sc.load(name))
    want = dc.coef_layout(info, want)
    for S in sc.SEGMENT_BYTES:
        call = sc.Call([name], S, 0)
        got = sc.decode(call)
        assert not got["status"].any() and not any(got["interval_status"]), (S, got["status"], got["interval_status"])
        assert np.array_equal(got["coef"][0].reshape(-1), want), S
        for row, entry in got["entries"].items():
            iv = interval(name, row)
            assert entry == iv.serial_entries(S), (S, row)
            assert entry[0] == (0, 0, 0) and all(0 <= e[1] < iv.bpm and 0 <= e[2] < 64 and e[0] <= iv.nbits for e in entry)
            assert got["rounds"][row] <= got["segments"][row] == iv.segments(S), (S, row, got["rounds"][row])
        assert sorted(got["entries"]) == list(range(len(call.desc)))


def test_a_threshold_between_the_interval_sizes_splits_only_the_long_ones():
    call = sc.Call(dc.MUTATED, 16, 0)
    sizes = sorted({int(v) for v in call.desc[:, 1]})
    call.split_min_bytes = sizes[len(sizes) // 2]
    got = sc.decode(call)
    assert not got["status"].any()
    split = [r >= 0 for r in got["rounds"]]
    assert split == [int(v) >= call.split_min_bytes for v in call.desc[:, 1]] and any(split) and not all(split)
    for i, name in enumerate(dc.MUTATED):
        info, want = dc.coefficients(dc.load(name))
        assert np.array_equal(got["coef"][i].reshape(-1), dc.coef_layout(info, want)), name


def test_slow_synchronisation_is_pinned():
    """Quality 100 on noise has almost no EOB, and the zigzag index only re-aligns at an EOB: at 8-byte segments the truth advances
    about a segment per round.  Correctness rests on iterating until nothing changes, not on luck."""
    got = sc.decode(sc.Call(["grey-16x24-q100-noise"], 8, 0))
    assert got["segments"][0] > 50 and got["rounds"][0] > got["segments"][0] // 2, (got["rounds"], got["segments"])
    assert got["rounds"][0] <= got["segments"][0]


def test_without_the_lenient_rule_the_chains_die():
    """A speculative walk abandoned at its first error hands its successors a dead state, and the truth advances one segment per
    round; the lenient rule needs strictly fewer rounds and fewer walks, and both end at the same states."""
    iv = interval("444-33x33")
    for S in (8, 16):
        entry, _, rounds, walks = iv.synchronise(S)
        dead_entry, _, dead_rounds, dead_walks = iv.synchronise(S, lenient=False)
        assert entry == dead_entry == iv.serial_entries(S)
        assert dead_rounds > rounds and dead_walks > walks, (S, rounds, dead_rounds)
        assert dead_rounds > iv.segments(S) // 2 > rounds


def test_unstuffing_and_the_status_keys():
    assert sc.unstuff(b"\x12\xff\x00\x00\xff\x00") == (b"\x12\xff\x00\xff", False)
    assert sc.unstuff(b"\x12\xff\x00\x34\xff\xd0\x56") == (b"\x12\xff\x34", True)
    assert sc.unstuff(b"\x12\xff") == (b"\x12", True) and sc.unstuff(b"\xff\xff\x00") == (b"", True) and sc.unstuff(b"") == (b"", False)
    # the smallest (ordinal, phase, word) wins: a DC range error of a block in front of its own entropy error, which is in front of
    # its sum, and all of them in front of anything in a later block
    assert min([(3, 1, dc.BAD_CODE), (3, 0, dc.COEF_RANGE), (2, 2, dc.COEF_RANGE), (7, 0, dc.NOT_CONSUMED)])[2] == dc.COEF_RANGE
    call = sc.Call(["420-33x33"], 8, 0)
    call.desc[0, 1] -= 40                                                   # the stream ends inside an MCU
    got = sc.decode(call)
    assert got["status"][0] == dc.TRUNCATED
    call = sc.Call(["420-33x33"], 8, 0)
    call.data[int(call.desc[0, 0]) + 100] = 0xFF
    call.data[int(call.desc[0, 0]) + 101] = 0xD0                            # a marker inside the interval
    assert sc.decode(call)["status"][0] != 0


def test_the_entry_points_are_declared():
    from streamflow_amd import _lib, build, jpeg_gpu, ops
    import inspect
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    for name in ("sf_jpeg_decode_split", "sf_jpeg_decode_split_ws_bytes"):
        assert name in _lib.SIGNATURES and name + "(" in hdr
    assert len(_lib.SIGNATURES["sf_jpeg_decode_split"][1]) == 22 and len(_lib.SIGNATURES["sf_jpeg_decode_split_ws_bytes"][1]) == 9
    assert any(h.endswith("jpeg_sync_core.h") for h in build.HEADERS)
    assert {"segment_bytes", "split_min_bytes"} <= set(inspect.signature(ops.jpeg_decode).parameters)
    assert {"split", "segment_bytes"} <= set(inspect.signature(jpeg_gpu.decode_batch).parameters) and jpeg_gpu.SPLIT_MIN_BYTES >= 1
    with pytest.raises(ValueError):
        jpeg_gpu.decode_batch([dc.load("444-8x8")], "cpu", split="sometimes")
    # at the default threshold no existing fixture and none of the project's own per-row files changes route
    assert max(len(dc.load(n)) for n in dc.NAMES) < jpeg_gpu.SPLIT_MIN_BYTES
