"""CPU: the decoder core the inflate kernel shares (csrc/inflate_core.h) as a stand-alone host program with a serial emit policy
(csrc/host/inflate_host_main.cpp), compiled with -fsanitize=address,undefined and run as its own process: nothing is preloaded and
nothing is loaded into Python.  Every stream gets heap buffers of exactly its input and output size, so invariant (a) -- no read
outside the input, no write outside the slot -- is the sanitizer's to check, and invariant (b) -- the decoder ends -- the process's.
Good and bad streams first, then a seeded sweep of single-byte substitutions and truncations, whose status must be 0 exactly where
zlib inflates the mutated stream to the same bytes.  Mutated streams go to this program only, never to a GPU."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import flo5_decode_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "streamflow_amd", "csrc", "host", "inflate_host_main.cpp")


def _clang():
    from streamflow_amd import build
    cands = [os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin", "clang++"),
             "/opt/rocm/lib/llvm/bin/clang++"]
    return next((c for c in cands if os.path.exists(c)), None) or shutil.which("clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _clang()
    assert cc, "the ROCm clang++ is needed to build the host program"
    exe = str(tmp_path_factory.mktemp("inflate_host") / "inflate_host")
    r = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", SRC,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, cases, tmp_path, tag):
    """cases: [(stream, expected length, stored flag)] -> [(status, output bytes)]; the run must be clean."""
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for s, n, stored in cases:
            f.write(struct.pack("<qqi", len(s), n, stored) + bytes(s))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    res, p, out = open(fout, "rb").read(), 0, []
    for _, n, _ in cases:
        out.append((struct.unpack_from("<i", res, p)[0], res[p + 4:p + 4 + n]))
        p += 4 + n
    assert p == len(res)
    return out


def test_good_and_bad_streams(program, tmp_path):
    good, bad = dc.good_streams(), dc.bad_streams()
    cases = [(s, len(d), 0) for _, s, d in good] + [(s, n, 0) for _, s, n, _ in bad]
    # stored as is: the right length, one too long, one too short
    raw = bytes(range(200))
    cases += [(raw, 200, 1), (raw, 199, 1), (raw, 201, 1), (b"", 0, 1)]
    got = _run(program, cases, tmp_path, "fixed")
    for (name, _, d), (st, out) in zip(good, got):
        assert st == dc.OK and out == d, (name, st)
    for (name, _, _, want), (st, _) in zip(bad, got[len(good):]):
        assert st == want, (name, dc.STATUS_NAMES[st], dc.STATUS_NAMES[want])
    tail = got[len(good) + len(bad):]
    assert [st for st, _ in tail] == [dc.OK, dc.OUTPUT_LONG, dc.OUTPUT_SHORT, dc.OK] and tail[0][1] == raw


SWEEP = ("text-l5-default", "text-l9-fixed", "text-flushes", "n64-l0-default", "skew-l9-huffman", "writer-37x53-c0")


def test_mutation_sweep(program, tmp_path):
    """2 000 single-byte substitutions and 200 truncations of each of six good streams: the program exits clean on every one, and
    its status is 0 exactly where zlib.decompressobj reaches the end of the stream with the expected length -- and then the bytes are
    zlib's.  (Nearly always those are the original bytes too; a few substitutions in the Huffman-only stream of small values change
    symbols in a way the Adler-32 does not see -- zlib accepts them with other bytes, and so must any decoder: 4 of these 13 200.)"""
    rng = np.random.default_rng(20261019)
    cases, want = [], []
    for name in SWEEP:
        s, d = dc.good(name)
        muts = []
        for _ in range(2000):
            i = int(rng.integers(0, len(s)))
            muts.append(s[:i] + bytes([(s[i] + int(rng.integers(1, 256))) & 255]) + s[i + 1:])
        muts += [s[:int(rng.integers(0, len(s)))] for _ in range(200)]
        for m in muts:
            cases.append((m, len(d), 0))
            do, z = zlib.decompressobj(), None
            try:
                z = do.decompress(m)
            except zlib.error:
                pass
            want.append(z if z is not None and do.eof and len(z) == len(d) else None)
    got = _run(program, cases, tmp_path, "sweep")
    assert len(got) == 6 * 2200
    wrong = [(k, st) for k, ((st, out), z) in enumerate(zip(got, want)) if (st == dc.OK) != (z is not None) or (z is not None and out != z)]
    assert not wrong, wrong[:10]
    same = sum(z is not None and z == dc.good(SWEEP[k // 2200])[1] for k, z in enumerate(want))
    accepted = sum(z is not None for z in want)
    assert accepted - same <= 8 and accepted < len(want) // 4                  # Adler-32 collisions are rare; most mutations fail
    assert len({st for st, _ in got}) >= 8                                     # the sweep reaches most of the failure codes
