"""What makes the assertions of tests/test_hip_conv_f32.py mean something, checked from the references alone (CPU).

Integer operands: the GPU test demands bit equality with float64.  That is only a fair demand while every partial
accumulation of the kernel, in whatever order it runs, is an integer below 2^24 -- the conv's own sums and the GroupNorm
partial rows.  Realistic operands: the GPU test's bound is e16 / 20; it separates an fp32 evaluation from any 16-bit operand
path only if fp32's own error sits far below e16.
"""
import pytest
import torch

from tests import conv_f32_cases as K

LIMIT = 2.0 ** 24
IDS = [K.case_id(c) for c in K.CASES]


def test_case_table_reaches_what_it_names():
    """The branches the table is there for, stated from the shapes: row counts, odd row count, both kernels, both
    strides, cout tiles of 1 / 2 / 4 and a cout that is no multiple of 32."""
    rows = [K.num_rows(c) for c in K.CASES]
    assert rows[0] == 2 and rows[1] == 3 and rows[2] == 8
    vox = [c[1][0] * c[1][1] * c[1][2] for c in K.CASES]
    plane = [c[1][1] * c[1][2] for c in K.CASES]
    assert 128 < vox[0] < 256                                      # case 0: the second half-tile is partly masked
    assert 256 // plane[1] + 1 == 7                                # case 1: a 256-voxel block spans 7 x-planes
    assert plane[2] % 256 != 0 and plane[2] > 256                  # case 2: blocks start in mid-plane
    assert {c[3] // 32 for c in K.CASES if c[3] % 32 == 0} == {1, 2, 4}
    assert {c[4] for c in K.CASES} == {1, 2, 3}
    assert any(c[3] % 32 for c in K.CASES)
    lds = [all(ch % 32 == 0 for ch, _ in c[2]) for c in K.CASES]
    assert lds.count(False) == 2 and lds.count(True) == 10
    for c in K.CASES:
        for (_, up), shp in zip(c[2], K.source_shapes(c)):
            if up:
                assert c[4] == 3 and all(v % 2 == 0 for v in c[1]) and shp[2:] == tuple(v // 2 for v in c[1])
    assert sum(ch for ch, _ in K.CASES[6][2]) * 27 == 6912


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_integer_operands_stay_exact_in_fp32(case):
    """conv(|x|, |w|) + |b| < 2^24 everywhere: every partial sum of the fmaf chain is an exact integer in any order.
    Per 128-voxel row and channel quad, sum |r| < 2^24 and sum r^2 < 2^24: so is every partial of the statistics.
    The operands are what the docstring of tests/conv_f32_cases.py says and the reference is integer-valued.
    Worst over the table: 5 801, 25 547 and 2.85e6 against 2^24 = 1.68e7."""
    srcs, w, b, y, rows = K.integer_expected(case)
    for t in srcs:
        assert t.min() >= -2 and t.max() <= 2 and torch.equal(t, t.round())
        assert len(t.unique()) == 5
    assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert b.abs().max() <= 4 and torch.equal(b, b.round())
    mag = K.conv64(case, [t.abs() for t in srcs], w.abs(), b.abs())
    assert mag.max().item() < LIMIT
    assert torch.equal(y, y.round()) and y.abs().max().item() <= mag.max().item()
    assert torch.equal(y.float().double(), y)
    if K.has_partials(case):
        a = K.row_sums(y.abs())[..., 0]
        print(f"{K.case_id(case)}: max sum|x||w|+|b| {mag.max().item():.0f}, row sum|r| {a.max().item():.0f}, "
              f"row sum r^2 {rows[..., 1].max().item():.0f}")
        assert a.max().item() < LIMIT and rows[..., 1].max().item() < LIMIT
        assert rows.shape == (case[0], K.num_rows(case), case[3] // 4, 2)
        assert torch.equal(rows, rows.round()) and torch.equal(rows.float().double(), rows)
        tot = y.reshape(case[0], case[3] // 4, -1)
        assert torch.equal(rows[..., 0].sum(dim=1), tot.sum(dim=-1))
        assert torch.equal(rows[..., 1].sum(dim=1), (tot * tot).sum(dim=-1))
    else:
        assert rows is None


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_realistic_bound_separates_fp32_from_16_bit_operands(case):
    """e32 (torch's fp32 CPU conv against float64) and e16 (the float64 conv of fp16-rounded activations and weights
    against float64), both over max(1, max |ref|): e16 >= 100 e32, so the GPU test's bound e16 / 20 leaves fp32 a factor
    of five and fails fp16 -- and bf16, three bits coarser -- by twenty.  Measured: e32 1.9e-7 .. 4.9e-7, e16 2.5e-4 .. 4.2e-4, ratio 630 .. 2050."""
    *_, e32, e16 = K.realistic_expected(case)
    print(f"{K.case_id(case)}: e32 {e32:.2e} e16 {e16:.2e} ratio {e16 / e32:.0f}")
    assert e32 > 0 and e16 >= 100 * e32

