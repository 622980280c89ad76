"""
The table-count guards of the fused-sumcheck wrappers (zkhip.api.Ctx): a wrong count is a ValueError BEFORE any pointer is laid out
for the C call, which reads exactly three numerators, three denominators, eleven / six / seven tables.  No GPU, no library: the
guards stand in front of everything that touches the context.
"""
import pytest

from zkhip.api import Ctx


@pytest.fixture(scope="module")
def ctx():
    return object.__new__(Ctx)  # no device behind it: a guard that let a call through would fail on the missing handle, not pass


@pytest.mark.parametrize("n_num, n_den", [(2, 4), (4, 2), (2, 3), (3, 4), (0, 6)])
def test_perm3_needs_three_and_three(ctx, n_num, n_den):
    nums, dens = [0] * n_num, [0] * n_den
    with pytest.raises(ValueError, match="three numerator and three denominator"):
        ctx.sumcheck_perm3(0, 0, nums, dens, 16, None, None)
    with pytest.raises(ValueError, match="three numerator and three denominator"):
        ctx.sumcheck_perm3_fs(0, 0, nums, dens, 16, None, None)


@pytest.mark.parametrize("name, need, gamma", [("gate_wide", 11, False), ("lookup", 6, True), ("lookup_sel", 7, True)])
def test_table_lists_need_their_exact_length(ctx, name, need, gamma):
    for count in (need - 1, need + 1):
        for suffix in ("", "_fs"):
            args = ([0] * count, 16) + ((None,) if gamma else ()) + (None,)
            with pytest.raises(ValueError, match="tables are needed"):
                getattr(ctx, f"sumcheck_{name}{suffix}")(*args)
