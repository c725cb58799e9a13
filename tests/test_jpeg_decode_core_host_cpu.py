"""CPU: the decoder core the JPEG entropy kernel shares (csrc/jpeg_decode_core.h) as a stand-alone host program with a serial policy
(csrc/host/jpeg_decode_host_main.cpp), compiled with -fsanitize=address,undefined and run as its own process: nothing is preloaded
and nothing is loaded into Python.  Data, descriptors, tables and the coefficient area are heap buffers of exactly their sizes, so
invariant (a) -- no read outside an interval's input, no write outside its blocks -- is the sanitizer's to check, and invariant (b)
-- the decoder ends -- the process's.  Valid files first (coefficients == decode_ref's walk), then the deterministic mutations of
jpeg_decode_cases.mutations() (the ones the GPU test repeats on the device) and a seeded sweep of byte substitutions, truncations
and random descriptor words that goes to this program only, never to a GPU."""
import numpy as np
import pytest

from tests import jpeg_decode_cases as dc


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return dc.host_program(tmp_path_factory.mktemp("jpeg_decode_host"))


def test_valid_files_give_the_reference_coefficients(program, tmp_path):
    calls = [dc.Call([n]) for n in dc.NAMES] + [dc.Call(dc.MUTATED)]
    got = dc.run_host(program, calls, tmp_path, "valid")
    for call, (status, ist, coef) in zip(calls, got):
        assert not status.any() and not ist.any(), (call.names, status, ist)
        for i, name in enumerate(call.names):
            info, want = dc.coefficients(dc.load(name))
            assert max(int(np.abs(c).max()) for c in want) <= dc.COEF_MAX
            assert max(int(np.abs(c).sum(axis=-1).max()) for c in want) <= dc.BLOCK_SUM_MAX
            assert np.array_equal(coef[i].reshape(-1), dc.coef_layout(info, want)), name


def test_deterministic_mutations_end_clean_with_a_status(program, tmp_path):
    """Image 1 of the batch is damaged; the program ends clean, images 0 and 2 keep status 0 and their coefficients, and the damage
    is reported under the expected word where the word is certain."""
    muts = dc.mutations()
    base = dc.run_host(program, [dc.Call(dc.MUTATED)], tmp_path, "base")[0]
    got = dc.run_host(program, [c for _, c in muts], tmp_path, "mutations")
    certain = {"into-the-next-marker": dc.BAD_MARKER, "all-ones-unstuffed": dc.BAD_MARKER, "lone-ff-at-the-end": dc.BAD_MARKER,
               "truncate-1000000": dc.TRUNCATED, "interval-missing": dc.BAD_DESC, "huffman-bits-all-255": dc.BAD_TABLE,
               "huffman-oversubscribed": dc.BAD_TABLE, "steps-of-255": dc.COEF_RANGE}
    seen = set()
    for (label, _), (status, _, coef) in zip(muts, got):
        # a row whose image is out of range is reported at the nearest image, and image 1 misses its MCUs
        want = {"image-past-the-batch": (0, dc.BAD_DESC), "image-negative": (dc.BAD_DESC, 0)}.get(label, (0, 0))
        assert (status[0], status[2]) == want, (label, status)
        assert np.array_equal(coef[0], base[2][0]) and np.array_equal(coef[2], base[2][2]), label
        if label in certain:
            assert status[1] == certain[label], (label, status)
        elif not label.startswith("flip-"):
            assert status[1] != 0, label
        if any(label.startswith(p) for p in ("in-", "image-", "first-", "n-mcus", "table-set")):
            assert status[1] == dc.BAD_DESC, (label, status)
        seen.add(int(status[1]))
    assert len(seen) >= 6, seen


def test_seeded_sweep(program, tmp_path):
    """400 single-byte substitutions and 100 truncations of each of five files, and 300 calls with one random descriptor word: the
    program exits clean on every one.  A file whose status is 0 after a substitution decoded to SOME coefficients inside the bounds;
    most substitutions fail."""
    rng = np.random.default_rng(20261021)
    calls = []
    for name in ("420-33x33", "444-16x17-q100-noise", "422-17x33-rst3", "grey-16x24-q100-checker", "own-basis77-only63-16x24"):
        base = dc.Call([name])
        for _ in range(400):
            c = base.copy()
            c.data[int(rng.integers(0, len(c.data)))] = int(rng.integers(0, 256))
            calls.append(c)
        for _ in range(100):
            c = base.copy()
            r = int(rng.integers(0, len(c.desc)))
            c.desc[r, 1] = int(rng.integers(0, c.desc[r, 1] + 1))
            calls.append(c)
    base = dc.Call(dc.MUTATED)
    for _ in range(300):
        c = base.copy()
        word = int(rng.integers(-2 ** 62, 2 ** 62)) if rng.integers(0, 2) else int(rng.integers(-20, 2000))
        c.desc[int(rng.integers(0, len(c.desc))), int(rng.integers(0, 6))] = word
        calls.append(c)
    got = dc.run_host(program, calls, tmp_path, "sweep")
    assert len(got) == 2800
    failed = sum(bool(status.any()) for status, _, _ in got)
    assert failed > len(got) // 2
    for status, _, coef in got:
        for i in np.flatnonzero(status == 0):
            assert int(np.abs(coef[i].astype(np.int64)).max()) <= dc.COEF_MAX
    assert len({int(s) for status, _, _ in got for s in status}) >= 7                  # the sweep reaches most of the status words
