"""tests/poison.py (the poisoned allocator the engine-state tests rely on) and EngineOptions.from_env, on the CPU.

The helper: tensors from torch.empty / torch.empty_like carry the byte in every format, zero-element tensors survive, torch.zeros
is untouched, the originals come back after a normal exit and after an exception, nesting is refused.  from_env: the bool
spellings, integer fields, `base` kept for the fields not named, the error for an unknown key, an empty or unset variable."""
from dataclasses import fields, replace

import numpy as np
import pytest
import torch

from tests import poison

DTYPES = (torch.float16, torch.float32, torch.float64, torch.uint8, torch.int64)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy()


@pytest.mark.parametrize("byte", poison.BYTES)
def test_empty_and_empty_like_carry_the_byte(byte):
    empty, empty_like = torch.empty, torch.empty_like
    with poison.poisoned(byte):
        assert torch.empty is not empty and torch.empty_like is not empty_like
        for dt in DTYPES:
            a = torch.empty(3, 5, dtype=dt)
            b = torch.empty((7,), dtype=dt, device="cpu")
            c = torch.empty_like(torch.ones(2, 3, 4, dtype=dt))
            d = torch.empty_like(torch.ones(4, 6, dtype=dt).t())                 # a non-contiguous model: the format is kept
            e = torch.empty_like(torch.ones(2, 2), dtype=dt)
            assert d.stride() == (1, 6)
            for t, shape in ((a, (3, 5)), (b, (7,)), (c, (2, 3, 4)), (d, (6, 4)), (e, (2, 2))):
                assert t.dtype == dt and tuple(t.shape) == shape
                got = _bytes(t)
                assert got.size == t.numel() * t.element_size() and (got == byte).all(), (dt, shape)
    assert torch.empty is empty and torch.empty_like is empty_like


def test_what_the_bytes_mean():
    """The reason for the three bytes: 0x00 is zero everywhere, 0xFF a NaN in every float format and -1 as an integer, 0x7B finite and
    huge -- and 0x7E, which older tests use, is a NaN as fp16."""
    with poison.poisoned(0x00):
        assert all(float(torch.empty(1, dtype=dt)[0]) == 0.0 for dt in DTYPES)
    with poison.poisoned(0xFF):
        assert all(torch.isnan(torch.empty(4, dtype=dt)).all() for dt in DTYPES[:3])
        assert int(torch.empty(1, dtype=torch.int64)[0]) == -1 and int(torch.empty(1, dtype=torch.uint8)[0]) == 255
    with poison.poisoned(0x7B):
        h, f, d = (torch.empty(1, dtype=dt) for dt in DTYPES[:3])
        assert float(h[0]) == 61280.0
        assert torch.isfinite(f).all() and 1.3e36 < float(f[0]) < 1.31e36
        assert torch.isfinite(d).all() and 6.5e286 < float(d[0]) < 6.6e286
    assert np.isnan(np.array([0x7E7E], np.uint16).view(np.float16)[0])


@pytest.mark.parametrize("byte", poison.BYTES)
def test_zero_element_tensors_and_zeros(byte):
    with poison.poisoned(byte):
        for shape in ((0,), (3, 0, 2), ()):
            for dt in DTYPES:
                t = torch.empty(shape, dtype=dt)
                assert tuple(t.shape) == shape and t.dtype == dt
        assert (_bytes(torch.empty((), dtype=torch.float64)) == byte).all()     # (a 0-dim tensor has one element)
        assert torch.empty_like(torch.ones(0, 4)).shape == (0, 4)
        z = torch.zeros(5, 7, dtype=torch.float16)
        assert not z.any() and not torch.zeros_like(torch.ones(3)).any()
        assert not torch.zeros(4, dtype=torch.int64).any()


def test_originals_restored_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    with pytest.raises(KeyError):
        with poison.poisoned(0xFF):
            assert torch.empty is not empty
            raise KeyError("body")
    assert torch.empty is empty and torch.empty_like is empty_like
    with poison.poisoned(0x7B):                                                 # ... and the helper can be entered again
        assert (_bytes(torch.empty(9)) == 0x7B).all()
    assert torch.empty is empty


def test_nesting_is_refused():
    empty = torch.empty
    with poison.poisoned(0xFF):
        inner = torch.empty
        with pytest.raises(RuntimeError, match="nesting"):
            with poison.poisoned(0x00):
                pass
        assert torch.empty is inner                                             # the refusal changed nothing
        assert (_bytes(torch.empty(3)) == 0xFF).all()
    assert torch.empty is empty
    with pytest.raises(ValueError):
        with poison.poisoned(256):
            pass
    assert torch.empty is empty


def test_fill_view_stays_inside_a_slice():
    buf = torch.zeros(64, dtype=torch.uint8)
    poison.fill_view(buf[8:24].view(torch.float32), 0xFF)
    want = np.zeros(64, np.uint8)
    want[8:24] = 0xFF
    assert (buf.numpy() == want).all()
    poison.fill_view(buf[:0], 0x7B)
    assert (buf.numpy() == want).all()


# ---- EngineOptions.from_env ------------------------------------------------------------------------------------------------------

def _options():
    from streamflow_amd.engine import EngineOptions
    return EngineOptions


def test_from_env_unset_or_empty_returns_base(monkeypatch):
    EngineOptions = _options()
    base = EngineOptions(split_solo=4, pw_fold=False, max_plans=2)
    monkeypatch.delenv("SF_ENGINE_OPTS", raising=False)
    assert EngineOptions.from_env(base) is base and EngineOptions.from_env() == EngineOptions()
    monkeypatch.setenv("SF_ENGINE_OPTS", "")
    assert EngineOptions.from_env(base) is base and EngineOptions.from_env(None) == EngineOptions()


@pytest.mark.parametrize("text,on", [("0", False), ("false", False), ("False", False), ("", False), ("1", True), ("true", True),
                                     ("True", True), ("yes", True), ("2", True), ("off", True), ("FALSE", True)])
def test_from_env_bool_spellings(monkeypatch, text, on):
    """Off is spelled 0, false, False or empty; anything else -- "off" and "FALSE" included -- is on."""
    EngineOptions = _options()
    for name, default in (("pw_fold", True), ("head_pairs", False)):
        monkeypatch.setenv("SF_ENGINE_OPTS", f"{name}={text}")
        for base in (None, EngineOptions(**{name: not default})):
            got = EngineOptions.from_env(base)
            assert getattr(got, name) is on
            assert got == replace(base or EngineOptions(), **{name: on})
    monkeypatch.setenv("SF_ENGINE_OPTS", " shadows = " + text + " ")          # blanks around key and value do not count
    assert EngineOptions.from_env().shadows is on
    if text == "":
        monkeypatch.setenv("SF_ENGINE_OPTS", "shadows")                         # no "=" at all: empty, off
        assert EngineOptions.from_env().shadows is False


def test_from_env_integers_and_base(monkeypatch):
    EngineOptions = _options()
    base = EngineOptions(parallel_branches=False, attn_k_splits=2, stored_auto_px=0, sk_tail_all=True)
    monkeypatch.setenv("SF_ENGINE_OPTS", "split_solo=0, attn_chunk_rows=96,max_plans= 1 ,pw_fold=0,head_pairs=1")
    got = EngineOptions.from_env(base)
    assert (got.split_solo, got.attn_chunk_rows, got.max_plans, got.pw_fold, got.head_pairs) == (0, 96, 1, False, True)
    assert type(got.split_solo) is int and type(got.pw_fold) is bool
    named = {"split_solo", "attn_chunk_rows", "max_plans", "pw_fold", "head_pairs"}
    for f in fields(EngineOptions):
        if f.name not in named:
            assert getattr(got, f.name) == getattr(base, f.name), f.name      # what the variable does not name is base's
    assert (got.parallel_branches, got.attn_k_splits, got.stored_auto_px, got.sk_tail_all) == (False, 2, 0, True)
    assert got != base and EngineOptions.from_env() == replace(EngineOptions(), split_solo=0, attn_chunk_rows=96, max_plans=1,
                                                                pw_fold=False, head_pairs=True)
    assert hash(got) != hash(base)                                              # every field is part of the graph key
    monkeypatch.setenv("SF_ENGINE_OPTS", "max_plans=two")
    with pytest.raises(ValueError):
        EngineOptions.from_env()


def test_from_env_every_field_is_reachable(monkeypatch):
    """Every field of the dataclass is a bool or an int and can be set from the variable (each one is part of the graph key)."""
    EngineOptions = _options()
    d = EngineOptions()
    for f in fields(EngineOptions):
        cur = getattr(d, f.name)
        assert type(cur) in (bool, int), f.name
        new = (not cur) if type(cur) is bool else cur + 1
        monkeypatch.setenv("SF_ENGINE_OPTS", f"{f.name}={int(new)}")
        got = EngineOptions.from_env()
        assert getattr(got, f.name) == new and type(getattr(got, f.name)) is type(cur), f.name
        assert got == replace(d, **{f.name: new})


def test_from_env_unknown_key_names_the_valid_ones(monkeypatch):
    EngineOptions = _options()
    monkeypatch.setenv("SF_ENGINE_OPTS", "pw_fold=0,split_sole=2")
    with pytest.raises(RuntimeError) as e:
        EngineOptions.from_env()
    msg = str(e.value)
    assert "split_sole" in msg
    for f in fields(EngineOptions):
        assert f.name in msg, f.name
