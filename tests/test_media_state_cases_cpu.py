"""The case table of the media state tests (tests/media_state_cases.py) on the CPU: every entry point of the C ABI is either in the
table or in COVERED_ELSEWHERE under an existing test, so a new entry point cannot be added without someone deciding which side it
belongs on; A is at least B in every buffer (sizes from the *_ws_bytes and bound functions, which load without a GPU); the content
variants keep every byte count; the split cases have an interval on either side of their threshold; every reference accepts what
it should and nothing launches."""
import os
import re

import numpy as np
import pytest

from tests import media_state_cases as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISSUE_LIST = ("sf_flow_consistency sf_warp_frames sf_frame_interp sf_resize_u8 sf_resize_f32 sf_jpeg_encode sf_jpeg_decode "
              "sf_jpeg_decode_split sf_flo5_encode sf_inflate sf_flo5_assemble sf_motion_moments sf_motion_solve sf_motion_fit "
              "sf_warp_affine_u8 sf_flow_to_kitti16 sf_png_encode sf_png_unfilter sf_frames_to_clips sf_clips_to_flows sf_tile_blend").split()


def test_every_entry_point_is_on_one_side_or_the_other():
    from streamflow_amd import _lib
    entry_points = [n for n in _lib.SIGNATURES if not n.endswith(mc.NOT_ENTRY_POINTS)]
    table, elsewhere = set(mc.ENTRIES), set(mc.COVERED_ELSEWHERE)
    assert len(mc.ENTRIES) == len(table) and sorted(table) == sorted(ISSUE_LIST)
    assert not table & elsewhere, table & elsewhere
    missing = [n for n in entry_points if n not in table and n not in elsewhere]
    assert not missing, f"neither in tests/media_state_cases.py's TABLE nor in COVERED_ELSEWHERE: {missing}"
    stale = [n for n in table | elsewhere if n not in entry_points]
    assert not stale, f"no such entry point: {stale}"
    print(f"{len(entry_points)} entry points: {len(table)} in the table, {len(elsewhere)} covered elsewhere")
    for name in sorted(entry_points):
        print(f"  {name}: {'TABLE' if name in table else mc.COVERED_ELSEWHERE[name]}")


def test_the_tests_named_for_the_others_exist():
    for name, where in mc.COVERED_ELSEWHERE.items():
        m = re.match(r"(tests/\w+\.py)(?:::(\w+))?", where)
        assert m, (name, where)
        path = os.path.join(REPO, m.group(1))
        assert os.path.exists(path) or m.group(1) == "tests/test_gpu_media_state.py", (name, where)
        if m.group(2):
            assert re.search(r"^def %s\(" % m.group(2), open(path).read(), re.M), (name, where)


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_a_is_at_least_b_in_every_buffer_and_the_variants_keep_the_sizes(entry):
    rec = mc.record(entry)
    a, b = rec.bind("A"), rec.bind("B")
    assert a.entry == b.entry == entry and list(a.bufs) == list(b.bufs)
    sa, sb = a.sizes(), b.sizes()
    assert all(v > 0 for v in sb.values()), sb
    assert all(sa[k] >= sb[k] for k in sa), (sa, sb)
    assert any(sa[k] > sb[k] for k in sa if a.bufs[k].role == mc.IN) and any(sa[k] > sb[k] for k in sa if a.bufs[k].role != mc.IN)
    assert [x.role for x in a.bufs.values()] == [x.role for x in b.bufs.values()]
    assert (mc.WS in [x.role for x in a.bufs.values()]) or not rec.int_ws
    for which, first in (("A", a), ("B", b)):
        seen = {tuple(bytes(x.data) for x in first.bufs.values() if x.role == mc.IN)}
        for v in range(1, mc.VARIANTS):
            other = rec.bind(which, v)
            assert other.sizes() == first.sizes(), (which, v)
            if which == "A":                                               # the replays need new content each; B runs as variant 0 only
                seen.add(tuple(bytes(x.data) for x in other.bufs.values() if x.role == mc.IN))
        assert which == "B" or len(seen) == mc.VARIANTS, f"{entry}: {len(seen)} distinct contents among {mc.VARIANTS} variants"


def test_the_split_cases_have_intervals_on_both_sides_of_the_threshold():
    for which in "AB":
        for v in range(mc.VARIANTS if which == "A" else 1):
            b = mc.bind_jpeg_decode_split(which, v)
            assert min(b.interval_bytes) < b.split_min_bytes <= max(b.interval_bytes), (which, b.split_min_bytes, b.interval_bytes)


def test_the_cases_with_class_maps_and_stats_are_there():
    for bind, names in ((mc.bind_frame_interp, ("cls_f", "cls_b", "stats", "cover")), (mc.bind_warp_frames, ("cls", "ref", "stats")),
                        (mc.bind_flow_consistency, ("cls", "stats")), (mc.bind_motion_moments, ("cls", "model", "inv_c2"))):
        for which in "AB":
            assert set(names) <= set(bind(which).bufs)


def test_references_accept_their_own_restatement_and_refuse_a_changed_byte():
    """check() on host-made outputs, where a module restates the output bytes directly: it passes on them and fails with one byte
    changed (the GPU module relies on check() to compare with the pinned reference)."""
    from tests import png_encode_cases as ec
    b = mc.bind_flow_to_kitti16("B")
    flow = b.bufs["flow"].data.view(np.float32).reshape(2, 2, 13, 37)
    good = mc.raw(np.stack([ec.kitti16_ref(f) for f in flow]))
    b.check({"out": good})
    bad = good.copy()
    bad[5] ^= 1
    with pytest.raises(AssertionError):
        b.check({"out": bad})
    b = mc.bind_frames_to_clips("B")
    lut = b.bufs["lut"].data.view(np.float32)
    assert lut[0] == -1.0 and lut[255] == 1.0 and len(lut) == 256
