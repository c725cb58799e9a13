"""CPU: corr.CorrPlan, the frozen record that keys a corr.CorrStore -- the arithmetic class it names, value semantics, and the store's
refusal of a form it does not know (raised before anything touches a device)."""
from dataclasses import FrozenInstanceError

import pytest

from streamflow_amd import ops
from streamflow_amd.corr import FORMS, CorrPlan, CorrStore


def test_prec_is_the_class_of_the_cells():
    assert FORMS == ("direct", "blocked16", "blocked32", "rows")
    for form in FORMS:
        for koct in (False, True):
            assert CorrPlan(form, True, koct).prec == ops.PRECISION_F16
            assert CorrPlan(form, False, koct).prec == ops.PRECISION_F16X3


def test_the_plan_is_a_frozen_value():
    a = CorrPlan("blocked16", True, True)
    assert a == CorrPlan("blocked16", True, koct_out=True) and hash(a) == hash(CorrPlan("blocked16", True, True))
    assert a != CorrPlan("blocked16", True, False) and a != CorrPlan("direct", True, True) and a != CorrPlan("blocked16", False, True)
    with pytest.raises(FrozenInstanceError):
        a.form = "rows"


def test_the_store_refuses_an_unknown_form():
    with pytest.raises(RuntimeError, match="form must be one of"):
        CorrStore(CorrPlan("volume", False, False), 1, 1, 256, 16, 24, "cpu")
