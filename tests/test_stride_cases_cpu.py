"""tests/stride_cases.py on the host: the embedding gives the alignment and slack it promises, and
its two checks catch the addressing mistakes the GPU tests (tests/test_gpu_strides.py) exist for —
emulated here by flat index arithmetic on a CPU tensor, the way a kernel addresses the buffer."""
import pytest

torch = pytest.importorskip("torch")

import stride_cases as SC  # noqa: E402

ROWS, COLS = 6, 8


def embedded(even):
    mat = torch.arange(1.0, ROWS * COLS + 1, dtype=torch.float64).reshape(ROWS, COLS)
    e = SC.embed(mat, even)
    base = e.top * e.ld + e.c0        # the operand's first element, in doubles from the buffer's start
    return mat, e, e.buf.view(-1), base


@pytest.mark.parametrize("even", [True, False])
def test_layout(even):
    mat, e, flat, base = embedded(even)
    assert e.ld == (COLS + 4 if even else COLS + 3) and e.c0 == (2 if even else 1)
    assert e.view.data_ptr() % 32 == 16 if even else e.view.data_ptr() % 16 == 8
    assert e.top >= ROWS + 1 and e.buf.shape[0] - e.top - ROWS >= ROWS       # guard rows above and below
    assert torch.equal(e.view, mat) and flat[base + 3 * e.ld + 5] == mat[3, 5]
    assert int(SC.is_sentinel(e.buf).sum()) == e.buf.numel() - ROWS * COLS
    assert bool(torch.isnan(e.buf[e.mask]).all())
    e.assert_slack_intact()


@pytest.mark.parametrize("even", [True, False])
def test_a_correct_kernel_passes(even):
    mat, e, flat, base = embedded(even)
    for i in range(ROWS):
        for j in range(COLS):
            flat[base + i * e.ld + j] *= 2.0
    e.assert_slack_intact()
    assert SC.same_bits(e.view, 2.0 * mat)


@pytest.mark.parametrize("even", [True, False])
def test_row_length_used_as_leading_dimension_is_caught(even):
    mat, e, flat, base = embedded(even)
    # a read with the wrong stride takes sentinels in: the result is NaN from the second row on
    got = torch.stack([flat[base + i * COLS:base + i * COLS + COLS] for i in range(ROWS)])
    assert torch.equal(got[0], mat[0]) and bool(torch.isnan(got[1:]).any())
    # a write with the wrong stride lands in a row's slack (never outside the buffer)
    for i in range(ROWS):
        flat[base + i * COLS:base + i * COLS + COLS] = 0.0
    with pytest.raises(AssertionError, match="sentinel"):
        e.assert_slack_intact()


@pytest.mark.parametrize("even", [True, False])
@pytest.mark.parametrize("where", ["past the last column", "before the first column", "row above", "row below"])
def test_one_store_outside_the_operand_is_caught(even, where):
    _, e, flat, base = embedded(even)
    off = {"past the last column": 2 * e.ld + COLS, "before the first column": 2 * e.ld - 1,
           "row above": -e.ld + 3, "row below": ROWS * e.ld + 3}[where]
    flat[base + off] = 0.0
    with pytest.raises(AssertionError, match="sentinel"):
        e.assert_slack_intact()


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = SC.sentinel_buffer((4,), "cpu")
    b = torch.full((4,), float("nan"), dtype=torch.float64)
    assert SC.same_bits(a, a.clone()) and not SC.same_bits(a, b)
    assert not SC.same_bits(torch.zeros(2, dtype=torch.float64), -torch.zeros(2, dtype=torch.float64))
    assert not bool(SC.is_sentinel(b).any()) and bool(SC.is_sentinel(a).all())
