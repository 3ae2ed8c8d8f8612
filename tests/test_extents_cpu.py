"""CPU suite: the arena of tests/extents.py must be able to fail.  Fake "kernels" written in torch plant one defect each on an
Arena("cpu"); verify() and the filler comparison must flag each one and name the operand and the side, and a correct fake passes."""
import pytest
import torch

import extents as E

ROWS, COLS, LD = 5, 12, 20
DTYPES = [torch.bfloat16, torch.float32, torch.int8]


def _flat(arena, view, cols):
    """the arena's memory from the operand's first element on, as elements of its dtype (what a kernel's pointer arithmetic sees)"""
    item = view.element_size()
    off = view.data_ptr() - arena.buf.data_ptr()
    return arena.buf[off:off + (arena.cur - off) // item * item].view(view.dtype)


def _before(arena, view, k):
    """the element k places in front of the operand's first one"""
    item = view.element_size()
    off = view.data_ptr() - arena.buf.data_ptr()
    return arena.buf[off - k * item:off - (k - 1) * item].view(view.dtype)


def _x(dtype):
    g = torch.Generator().manual_seed(3)
    return torch.randint(-9, 10, (ROWS, COLS), generator=g).to(dtype)


def fake(defect, dtype=torch.bfloat16):
    """y = 2 x on strided operands, with one planted defect"""
    def run(arena):
        (_, x), = [arena.place(_x(dtype), ld=LD, role="in", name="x")]
        _, y = arena.place(torch.empty(ROWS, COLS, dtype=dtype), ld=LD, role="out", name="y")
        arena.arm()
        y.copy_((x.float() * 2).to(dtype))
        mem_y, mem_x = _flat(arena, y, COLS), _flat(arena, x, COLS)
        if defect == "past_last_row":
            mem_y[ROWS * LD] = 3
        elif defect == "row_gap":
            mem_y[2 * LD + COLS + 1] = 3
        elif defect == "in_front":
            _before(arena, y, 2)[0] = 3
        elif defect == "input_modified":
            x[1, 4] = 7 if float(x[1, 4]) != 7 else 6
        elif defect == "element_skipped":
            y[3, 7:8].view(E._RAW[y.element_size()]).copy_(E.unwritten_value(dtype).view(E._RAW[y.element_size()]))
        elif defect == "zero_times_past_the_input":
            y[ROWS - 1, 0] = (y[ROWS - 1, 0].float() + 0.0 * mem_x[ROWS * LD].float()).to(dtype)       # the element just past the input
        else:
            assert defect is None
        return {"y": y}
    return run


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_correct_fake_passes(dtype):
    out = E.filler_passes(fake(None, dtype), "cpu", capacity=1 << 20)
    assert torch.equal(out["y"].float(), _x(dtype).float() * 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect,operand,words", [
    ("past_last_row", "y", f"behind the operand, row {ROWS}, col 0"),
    ("row_gap", "y", f"gap between rows, row 2, col {COLS + 1}"),
    ("in_front", "y", "in front of the operand, 2 element(s) before its start (row -1, col 18)"),
    ("input_modified", "x", "input modified at row 1, col 4"),
    ("element_skipped", "y", "output element never written at row 3, col 7"),
])
def test_verify_names_the_operand_and_the_side(defect, operand, words, dtype):
    with pytest.raises(E.ExtentError) as e:
        E.filler_passes(fake(defect, dtype), "cpu", capacity=1 << 20, passes=("tame",))
    assert str(e.value).startswith(operand + ":") and words in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_read_past_the_input_multiplied_by_zero_shows_in_the_filler_comparison(dtype):
    """0 * 1.0 is 0: the tame runs pass.  0 * NaN is NaN: the NaN run differs, in the last row's first element."""
    E.filler_passes(fake("zero_times_past_the_input", dtype), "cpu", capacity=1 << 20, passes=("tame", "tame"))
    for hostile in ("nan", "inf"):
        with pytest.raises(E.ExtentError) as e:
            E.filler_passes(fake("zero_times_past_the_input", dtype), "cpu", capacity=1 << 20, passes=("tame", hostile))
        assert str(e.value).startswith("y:") and f"({hostile} filler)" in str(e.value) and f"row {ROWS - 1}, col 0" in str(e.value), str(e.value)


def test_a_run_that_is_not_repeatable_is_told_from_a_filler_dependence():
    n = [0]

    def run(arena):
        out = fake(None)(arena)
        n[0] += 1
        out["y"][0, 0] += n[0]
        return out
    with pytest.raises(E.ExtentError, match="not deterministic"):
        E.filler_passes(run, "cpu", capacity=1 << 20)


def test_a_refused_call_must_leave_its_outputs_alone():
    def run(arena, write):
        _, y = arena.place(torch.empty(ROWS, COLS), ld=LD, role="out", name="y")
        arena.arm()
        arena.refused = True
        if write:
            y[2, 3] = 1.0
        return {}
    E.filler_passes(lambda a: run(a, False), "cpu", capacity=1 << 20, passes=("tame",))
    with pytest.raises(E.ExtentError, match="y: output written by a refused call at row 2, col 3"):
        E.filler_passes(lambda a: run(a, True), "cpu", capacity=1 << 20, passes=("tame",))


def test_layout_conditions():
    """guards of at least 64 KiB, the back one at least 256 rows of the operand's stride; 256-byte aligned starts; the fused layout"""
    a = E.Arena("cpu", "nan", capacity=8 << 20)
    p0, v0 = a.place(torch.zeros(3, 16, dtype=torch.float32), ld=24, role="in")
    wide = torch.zeros(4, 1024, dtype=torch.bfloat16)
    (p1, q), (p2, k) = a.place_fused([wide, wide], ["inout", "in"], pad=8)
    assert p0 % 256 == 0 and p1 % 256 == 0 and p2 == p1 + 2048 and q.stride(0) == k.stride(0) == 2056
    b0, b1 = a.buffers
    assert b0.front >= E.GUARD and b1.front >= E.GUARD and b0.back >= E.GUARD and b1.back >= 256 * 2056 * 2 > E.GUARD
    assert p1 - (p0 + 3 * 24 * 4) >= b0.back + E.GUARD
    assert bool(torch.isnan(a.buf[b0.off - b0.front:b0.off].view(torch.float32)).all())                 # hostile filler all round
    grid = a.buf[b0.off:b0.off + 3 * 24 * 4].view(torch.float32).view(3, 24)
    assert bool(torch.isnan(grid[:, 16:]).all()) and bool((v0 == 0).all())        # the row gap; the input
    i8 = E.Arena("cpu", "inf", capacity=1 << 20)
    _, v = i8.place(torch.zeros(2, 8, dtype=torch.int8), ld=16, role="out")
    assert bool((v == -128).all()) and int(i8.buf[i8.buffers[0].off + 8]) == 0x80
    with pytest.raises(RuntimeError, match="arm"):
        i8.verify()
    if E.F8 is not None:
        f8 = E.Arena("cpu", "tame", capacity=1 << 20)
        _, v = f8.place(torch.zeros(2, 8, dtype=torch.uint8).view(E.F8), ld=16, role="in")
        assert int(f8.buf[f8.buffers[0].off + 8]) == 0x38 and float(E.filler_value(E.F8, "tame").float()) == 1.0
