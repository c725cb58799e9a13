"""CPU: the cases of the .flo5 device reader hold what they claim (tests/flo5_decode_cases.py), flo5.chunk_table indexes every file
the reader reads, and the new switches and entry points are where the issue puts them.  No GPU."""
import glob
import os
import zlib

import numpy as np
import pytest
import torch

from tests import flo5_decode_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def test_inflate_ref_equals_zlib_on_good_streams():
    for name, s, d in dc.good_streams():
        assert zlib.decompress(s) == d, name
        got, st = dc.inflate_ref(s, len(d))
        assert st == dc.OK and got == d, (name, dc.STATUS_NAMES[st])


def test_inflate_ref_status_on_bad_streams():
    bad = dc.bad_streams()
    assert len(bad) == 12 and len({n for n, *_ in bad}) == 12
    for name, s, n, status in bad:
        assert status != dc.OK
        assert dc.inflate_ref(s, n)[1] == status, (name, dc.STATUS_NAMES[dc.inflate_ref(s, n)[1]])
        do = zlib.decompressobj()                                             # ... and zlib does not deliver n bytes from it either
        try:
            got = do.decompress(s)
            assert not (do.eof and len(got) == n), name
        except zlib.error:
            pass
    assert {b[3] for b in bad} >= {dc.BAD_HEADER, dc.TRUNCATED, dc.BAD_BLOCK_TYPE, dc.BAD_CODE_LENGTHS, dc.BAD_DISTANCE, dc.OUTPUT_LONG,
                                   dc.OUTPUT_SHORT, dc.BAD_ADLER, dc.BAD_STORED_LEN, dc.PRESET_DICT}


def test_good_streams_cover_every_feature():
    """The list as a whole holds everything sf_inflate must decode; losing the only stream with one of them fails here."""
    f = dc.features()
    assert f["types"] == {0, 1, 2}                                            # stored, fixed, dynamic
    assert f["repeats"] == {16, 17, 18}
    assert f["max_code_len"] == 15
    assert f["max_dist"] == 32768
    assert f["overlap"]                                                       # distance < length
    assert f["blocks"] >= 3                                                   # several blocks in one stream
    assert f["empty_stored"] >= 1 and f["max_stored_len"] == 65535
    assert f["zero_output"]
    names = [n for n, _, _ in dc.good_streams()]
    assert len(set(names)) == len(names)
    for level in (0, 1, 5, 9):
        for strat in ("default", "fixed", "huffman", "rle"):
            assert f"text-l{level}-{strat}" in names
    assert any(n.startswith("writer-") for n in names) and len(dc.good("chunk-l5")[1]) == 65280


def _files():
    exp = np.load(os.path.join(GOLD, "flo5_decode", "expected.npz"))["field"]
    out = [(p, None) for p in sorted(glob.glob(os.path.join(GOLD, "flo5", "*.flo5")))]
    out += [(os.path.join(GOLD, "flo5_decode", "auto_gzip5.flo5"), exp), (os.path.join(GOLD, "flo5_decode", "shuffle_gzip9.flo5"), exp),
            (os.path.join(GOLD, "flo5_decode", "stored_gzip0.flo5"), exp[:136, :240])]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.dtype(f"u{a.dtype.itemsize}"))


def _via_table(table):
    chunks = dc.table_chunks(table)
    return dc.assemble_ref(table["shape"], table["chunk_shape"], 2 in table["filters"], chunks)


def test_chunk_table_on_golden_files():
    from streamflow_amd import flo5
    seen = set()
    for path, exp in _files():
        want = flo5.read_flo5(path)
        t = flo5.chunk_table(path)
        assert t["shape"] == want.shape and t["dtype"] == want.dtype and t["path"] == path
        if exp is not None:
            assert np.array_equal(_bits(want), _bits(exp)), path              # the reader against what h5py was given
        if not t["chunked"]:
            assert t["chunks"] == [] and t["chunk_shape"] is None
            seen.add("contiguous")
            continue
        assert want.dtype == np.float32
        for offs, addr, nbytes, mask in t["chunks"]:
            assert len(offs) == 3 and 0 <= addr and addr + nbytes <= len(t["data"]) and mask == 0
        assert np.array_equal(_via_table(t), _bits(want)), path
        seen.add((t["chunk_shape"][2], tuple(t["filters"])))
        with open(path, "rb") as f:                                           # the file's bytes instead of its path
            assert flo5.chunk_table(f.read())["chunks"] == t["chunks"]
    # channel-split chunks, whole-pixel chunks, a shuffle pipeline, an unchunked dataset: all met
    assert {"contiguous", (1, (1,)), (2, (1,)), (2, (2, 1)), (1, (2, 1))} <= seen, seen
    big = flo5.chunk_table(os.path.join(GOLD, "flo5_decode", "auto_gzip5.flo5"))
    assert big["chunk_shape"] == (34, 120, 1) and len(big["chunks"]) == 8 * 4 * 2 and big["filters"] == [1]
    with pytest.raises(IOError, match="does not have a 'nope' key"):
        flo5.chunk_table(os.path.join(GOLD, "flo5", "tiny_1x1.flo5"), "nope")
    with pytest.raises(IOError, match="not an HDF5 file"):
        flo5.chunk_table(b"\0" * 600)


TILED = [((37, 53), (19, 53, 2), 5, False, (), ()), ((136, 240), (34, 60, 1), 5, False, ((1, 2, 0),), ((3, 3, 1), (0, 0, 0))),
         ((33, 40), (8, 16, 2), 9, True, ((2, 1, 0),), ((4, 2, 0),)), ((70, 9), (3, 9, 2), 1, False, (), ())]


@pytest.mark.parametrize("case", TILED, ids=lambda c: "x".join(map(str, c[0] + c[1])))
def test_tiled_file_reads_back(case, tmp_path):
    from streamflow_amd import flo5
    (h, w), cs, level, shuffle, skip, missing = case
    a = dc.smooth_field(h, w, 3)
    blob = dc.tiled_file(a, cs, level, shuffle, skip, missing)
    p = str(tmp_path / "t.flo5")
    with open(p, "wb") as f:
        f.write(blob)
    want = a.copy()
    for gy, gx, gc in missing:
        want[gy * cs[0]:(gy + 1) * cs[0], gx * cs[1]:(gx + 1) * cs[1], gc * cs[2]:(gc + 1) * cs[2]] = 0.0
    got = flo5.read_flo5(p)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    t = flo5.chunk_table(blob)
    n_cells = -(-h // cs[0]) * -(-w // cs[1]) * (2 // cs[2])
    assert len(t["chunks"]) == n_cells - len(missing) and t["chunk_shape"] == cs
    assert sorted(m for *_, m in t["chunks"] if m) == [2 if shuffle else 1] * len(skip)
    assert np.array_equal(_via_table(t), _bits(want))
    if n_cells - len(missing) > 9:                                            # three entries per node: leaves, a middle level, a root
        assert blob[:t["chunks"][0][1]].count(b"TREE") >= 1 + 4 + 2 + 1


def test_flo5_decode_switch_is_checked():
    from streamflow_amd import evaluate
    stub = lambda *a, **k: None
    with pytest.raises(ValueError, match="flo5_decode must be"):
        evaluate.spring_report(stub, flo5_decode="device")
    with pytest.raises(ValueError, match="flo5_decode must be"):
        evaluate.validate_spring_mf(stub, flo5_decode="device")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.spring_report(stub, device=torch.device("cpu"), flo5_decode="gpu")
    with pytest.raises(ValueError, match="inflate must be"):
        from streamflow_amd import flo5_gpu
        flo5_gpu.read_batch(["x.flo5"], "cuda", inflate="device")


def test_command_line_lists_flo5_decode(capsys):
    from streamflow_amd import evaluate
    with pytest.raises(SystemExit):
        evaluate.main(["--help"])
    assert "--flo5-decode" in capsys.readouterr().out


def test_entry_points_are_declared_everywhere():
    from streamflow_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    for name in ("sf_inflate", "sf_flo5_assemble"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
    assert "flo5_decode.hip" in build.SOURCES and any(h.endswith("inflate_core.h") for h in build.HEADERS)
    assert "inflate_kernel" in build.HOT_KERNELS and "flo5_assemble_kernel" in build.HOT_KERNELS
    # the status words: header, core and the Python names agree
    import re
    words = dict((n, int(v)) for n, v in re.findall(r"SF_INFLATE_([A-Z_]+) = (\d+)", hdr))
    assert [words[n] for n in dc.STATUS_NAMES] == list(range(13)) and len(ops.INFLATE_STATUS) == 13
    core = open(os.path.join(build.CSRC, "inflate_core.h")).read()
    for n in dc.STATUS_NAMES:
        camel = "k" + "".join(p.capitalize() for p in n.split("_"))
        assert re.search(rf"{camel} = {words[n]}\b", core), camel
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.inflate(torch.zeros(4, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int64), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flo5_assemble(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 1, 1, 1, dtype=torch.int32), 1, 1, (1, 1, 2), False)


def test_argument_validation_of_the_entry_points():
    """sf_inflate / sf_flo5_assemble refuse what they cannot run before any launch (dummy, never dereferenced pointers)."""
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    P = 0x10000
    assert lib.sf_inflate(None, 8, P, 1, P, 8, P, None) == -1 and b"null" in lib.sf_last_error()
    assert lib.sf_inflate(P, 8, P, 0, P, 8, P, None) == -1 and b"n = 0" in lib.sf_last_error()
    assert lib.sf_inflate(P, -1, P, 1, P, 8, P, None) == -1 and b"negative" in lib.sf_last_error()
    assert lib.sf_inflate(P, 8, P + 4, 1, P, 8, P, None) == -1 and b"desc is not 8-byte aligned" in lib.sf_last_error()
    assert lib.sf_inflate(P, 8, P, 1, P, 8, P + 2, None) == -1 and b"status is not 4-byte aligned" in lib.sf_last_error()
    ok = dict(chunks=P, chunk_stride=64, n_slots=1, grid=P, n=1, h=2, w=2, ch=2, cw=2, cc=2, shuffle=0, out=P)
    call = lambda **kw: lib.sf_flo5_assemble(*{**ok, **kw}.values(), None)
    assert call(grid=None) == -1 and b"null" in lib.sf_last_error()
    assert call(n=0) == -1 and b"n = 0" in lib.sf_last_error()
    assert call(n=65536) == -1 and call(h=65536) == -1 and call(w=0) == -1
    assert call(cc=3) == -1 and b"cc must be 1 or 2" in lib.sf_last_error()
    assert call(chunk_stride=28) == -1 and call(chunk_stride=62) == -1 and b"chunk_stride" in lib.sf_last_error()
    assert call(n_slots=-1) == -1 and call(chunks=P + 2) == -1 and call(out=P + 4) == -1 and b"8-byte aligned" in lib.sf_last_error()
    assert call(ch=1 << 15, cw=1 << 15, chunk_stride=1 << 40) == -1 and b"2^31" in lib.sf_last_error()
