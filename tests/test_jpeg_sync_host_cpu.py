"""CPU: the functions the split route's kernels run (csrc/jpeg_sync_core.h) as a stand-alone host program
(csrc/host/jpeg_sync_host_main.cpp: phase by phase, segment by segment), compiled with -fsanitize=address,undefined and run as its
own process: nothing is preloaded and nothing is loaded into Python.  Data, descriptors, tables, the coefficient area and every
interval's unstuffed stream are heap buffers of exactly their sizes, so invariant (a) is the sanitizer's to check and invariant (b)
-- every walk and every window's rounds end -- the process's.  Valid files first (coefficients == the serial host program's and
the Python restatement's rounds), then the deterministic mutations of jpeg_decode_cases.mutations() (the ones the GPU test repeats
on the device) and a seeded sweep of the make-up of test_jpeg_decode_core_host_cpu.test_seeded_sweep that goes to this program
only, never to a GPU."""
import numpy as np
import pytest

from tests import jpeg_decode_cases as dc
from tests import jpeg_sync_cases as sc


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return sc.host_program(tmp_path_factory.mktemp("jpeg_sync_host"))


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    return dc.host_program(tmp_path_factory.mktemp("jpeg_decode_host"))


def test_valid_files_give_the_serial_programs_coefficients(program, serial, tmp_path):
    names = [[n] for n in sc.NAMES] + [list(dc.MUTATED)]
    want = dc.run_host(serial, [sc.Call(n) for n in names], tmp_path, "serial")
    for S in sc.SEGMENT_BYTES:
        calls = [sc.Call(n, S, 0) for n in names]
        got = sc.run_host(program, calls, tmp_path, f"valid{S}")
        for call, g, (status, ist, coef) in zip(calls, got, want):
            assert not status.any() and not g["status"].any() and not g["interval_status"].any(), (call.names, S, g["status"])
            assert np.array_equal(g["coef"], coef), (call.names, S)
            assert (g["rounds"] >= 0).all() and (g["rounds"] <= g["segments"]).all(), (call.names, S, g["rounds"], g["segments"])
    # the rounds are the restatement's: the same method, not merely the same result
    for name in ("grey-16x24-q100-noise", "420-33x33", "444-8x2736", "sync-420-96x128-q90"):
        g = sc.run_host(program, [sc.Call([name], 8, 0)], tmp_path, "rounds")[0]
        r = sc.decode(sc.Call([name], 8, 0))
        assert (list(g["rounds"]), list(g["redecodes"]), list(g["segments"])) == (r["rounds"], r["redecodes"], r["segments"]), name


def test_a_threshold_mixes_both_routes(program, serial, tmp_path):
    base = sc.Call(dc.MUTATED, 16, 0)
    sizes = sorted({int(v) for v in base.desc[:, 1]})
    base.split_min_bytes = sizes[len(sizes) // 2]
    never = sc.Call(dc.MUTATED, 16, len(base.data) + 1)
    want = dc.run_host(serial, [base], tmp_path, "serial")[0]
    mixed, none = sc.run_host(program, [base, never], tmp_path, "mixed")
    assert [r >= 0 for r in mixed["rounds"]] == [int(v) >= base.split_min_bytes for v in base.desc[:, 1]]
    assert 0 < int((mixed["rounds"] >= 0).sum()) < len(base.desc) and (none["rounds"] == -1).all()
    for g in (mixed, none):
        assert not g["status"].any() and np.array_equal(g["coef"], want[2])


def test_deterministic_mutations_end_clean_with_the_serial_programs_verdict(program, serial, tmp_path):
    """Image 1 of the batch is damaged.  At every segment size the program ends clean, every image's status is zero exactly where
    the serial program's is, images 0 and 2 keep their coefficients, and the `certain` labels of the serial program's test give
    the same words."""
    muts = dc.mutations()
    assert len(muts) == 34
    base = dc.run_host(serial, [dc.Call(dc.MUTATED)], tmp_path, "base")[0]
    want = dc.run_host(serial, [c for _, c in muts], tmp_path, "serial")
    certain = {"into-the-next-marker": dc.BAD_MARKER, "all-ones-unstuffed": dc.BAD_MARKER, "lone-ff-at-the-end": dc.BAD_MARKER,
               "truncate-1000000": dc.TRUNCATED, "interval-missing": dc.BAD_DESC, "huffman-bits-all-255": dc.BAD_TABLE,
               "huffman-oversubscribed": dc.BAD_TABLE, "steps-of-255": dc.COEF_RANGE}
    for S in sc.SEGMENT_BYTES:
        got = sc.run_host(program, [sc.Call.of(c, S, 0) for _, c in muts], tmp_path, f"mutations{S}")
        for (label, _), g, (status, _, _) in zip(muts, got, want):
            assert np.array_equal(g["status"] == 0, status == 0), (label, S, g["status"], status)
            for i in (0, 2):
                if status[i] == 0:
                    assert np.array_equal(g["coef"][i], base[2][i]), (label, S, i)
            if label in certain:
                assert g["status"][1] == certain[label], (label, S, g["status"])
            if any(label.startswith(p) for p in ("in-", "image-", "first-", "n-mcus", "table-set")):
                assert g["status"][1] == dc.BAD_DESC, (label, S, g["status"])


def test_seeded_sweep(program, serial, tmp_path):
    """400 single-byte substitutions and 100 truncations of each of five files, and 300 calls with one random descriptor word, every
    interval split at 8-byte segments (16 for the descriptor words): the program exits clean on every one, every image's status is
    zero exactly where the serial program's is, and then the coefficients are the serial program's."""
    rng = np.random.default_rng(20261021)
    calls = []
    for name in ("420-33x33", "444-16x17-q100-noise", "422-17x33-rst3", "grey-16x24-q100-checker", "own-basis77-only63-16x24"):
        base = sc.Call([name], 8, 0)
        for _ in range(400):
            c = base.copy()
            c.data[int(rng.integers(0, len(c.data)))] = int(rng.integers(0, 256))
            calls.append(c)
        for _ in range(100):
            c = base.copy()
            r = int(rng.integers(0, len(c.desc)))
            c.desc[r, 1] = int(rng.integers(0, c.desc[r, 1] + 1))
            calls.append(c)
    base = sc.Call(dc.MUTATED, 16, 0)
    for _ in range(300):
        c = base.copy()
        word = int(rng.integers(-2 ** 62, 2 ** 62)) if rng.integers(0, 2) else int(rng.integers(-20, 2000))
        c.desc[int(rng.integers(0, len(c.desc))), int(rng.integers(0, 6))] = word
        calls.append(c)
    got = sc.run_host(program, calls, tmp_path, "sweep")
    want = dc.run_host(serial, calls, tmp_path, "serial")
    assert len(got) == 2800
    assert sum(bool(g["status"].any()) for g in got) > len(got) // 2
    for k, (g, (status, _, coef)) in enumerate(zip(got, want)):
        assert np.array_equal(g["status"] == 0, status == 0), (k, g["status"], status)
        for i in np.flatnonzero(status == 0):
            assert np.array_equal(g["coef"][i], coef[i]), (k, i)
    assert len({int(s) for g in got for s in g["status"]}) >= 7
