"""CPU: what the host side of the grid searches shares (nfopp/_grid.py) on torch CPU tensors and numpy arrays -- the goal
table against np.unique, the sized trace against a fake field / trace pair that records its calls, the frame against
tests/grid_search_ref.py and the numpy expression of the reference, and the workspace.  No GPU and no library call."""
import ctypes

import numpy as np
import pytest
import torch

from nfopp import _grid

import grid_search_ref as gsr


# ---- goal_table ------------------------------------------------------------------------------------------------------------
def _goal_table_ref(key):
    """np.unique restated: the distinct keys without -1, and each problem's entry among them (-1 for a key of -1)."""
    key = np.asarray(key, np.int64)
    uniq = np.unique(key[key >= 0])
    index = np.where(key >= 0, np.searchsorted(uniq, key), -1)
    return uniq, index


@pytest.mark.parametrize("key", [[], [-1, -1, -1], [5, 0, 5, 9, 2], [7, -1, 3, 7, -1]],
                         ids=["B=0", "every goal outside", "no goal outside", "two of five outside"])
def test_goal_table_is_np_unique_without_the_outside_key(key):
    uniq, field_index = _grid.goal_table(torch.tensor(key, dtype=torch.int64))
    want_uniq, want_index = _goal_table_ref(key)
    assert uniq.dtype == torch.int64 and field_index.dtype == torch.int32 and field_index.is_contiguous()
    assert uniq.shape == (len(want_uniq),) and field_index.shape == (len(key),)
    assert np.array_equal(uniq.numpy(), want_uniq) and np.array_equal(field_index.numpy(), want_index)


def test_goal_table_of_the_stated_five_problems():
    uniq, field_index = _grid.goal_table(torch.tensor([7, -1, 3, 7, -1]))
    assert uniq.tolist() == [3, 7] and field_index.tolist() == [1, -1, 0, 1, -1]
    uniq, field_index = _grid.goal_table(torch.tensor([-1, -1], dtype=torch.int64))
    assert uniq.numel() == 0 and field_index.tolist() == [-1, -1]


def test_cell_keys_flags_the_cells_outside():
    cells = torch.tensor([[0, 0], [2, 4], [-1, 0], [3, 0], [0, 5], [1, -1]], dtype=torch.int32)
    inside, flat = _grid.cell_keys(cells, (3, 5))
    assert inside.tolist() == [True, True, False, False, False, False] and flat.dtype == torch.int64
    assert flat[:2].tolist() == [0, 14]


# ---- the sized trace -------------------------------------------------------------------------------------------------------
class FakeSearch(object):
    """A field / trace pair for traced_search: problem p belongs to field p % n_fields and its path has lengths[p] states.  A
    sizing pass writes the counts of the chunk's problems; a filling pass asserts that every buffer holds the largest count seen
    so far and writes p + 1 into the first lengths[p] entries of every buffer.  Every call is recorded."""

    def __init__(self, lengths, n_fields):
        self.lengths, self.n_fields, self.calls, self.largest, self.buffers = list(lengths), n_fields, [], 0, []

    def fields_of(self, first, last):
        self.calls.append(("fields", first, last))
        return (first, last)

    def trace(self, fields, first, paths, count, status, cost):
        self.calls.append(("size" if paths is None else "fill", first))
        mine = [p for p in range(len(self.lengths)) if fields is not None and fields[0] <= p % self.n_fields < fields[1]]
        if fields is not None:
            assert fields[0] == first
        if paths is None:
            for p in mine:
                count[p] = self.lengths[p]
                status[p] = 0
            if fields is None:
                count.zero_()
                status.fill_(2)
            self.largest = max([self.largest] + [self.lengths[p] for p in mine])
            return
        self.buffers.append([t.shape[1] for t in paths])
        for t in paths:
            assert t.shape[1] >= max(self.largest, 1) and t.dtype == torch.int32 and t.is_contiguous()
            for p in mine:
                assert not t[p].any()                     # a grown buffer is zero where nothing was written
                t[p, :self.lengths[p]] = p + 1


def test_three_chunks_grow_the_buffers_and_never_shrink_them():
    lengths = [4, 2, 9, 3, 1, 5]                          # fields 0, 1, 2 hold the problems (0, 3), (1, 4), (2, 5): maxima 4, 2, 9
    fake = FakeSearch(lengths, 3)
    paths, count, status, cost = _grid.traced_search(6, "cpu", 3, 1, ((2,), ()), fake.fields_of, fake.trace)
    assert fake.calls == [("fields", 0, 1), ("size", 0), ("fill", 0), ("fields", 1, 2), ("size", 1), ("fill", 1),
                          ("fields", 2, 3), ("size", 2), ("fill", 2)]
    assert fake.buffers == [[4, 4], [4, 4], [9, 9]]
    cells, headings = paths
    assert cells.shape == (6, 9, 2) and headings.shape == (6, 9) and cost.shape == (6, 2)
    assert count.tolist() == lengths and status.tolist() == [0] * 6
    for p, n in enumerate(lengths):                       # what an earlier chunk filled survives the growth; zero behind the count
        assert headings[p].tolist() == [p + 1] * n + [0] * (9 - n)
        assert cells[p].tolist() == [[p + 1, p + 1]] * n + [[0, 0]] * (9 - n)


def test_two_fields_a_chunk_take_the_last_chunk_short():
    fake = FakeSearch([1, 2, 3], 3)
    paths, count, _, _ = _grid.traced_search(3, "cpu", 3, 2, ((),), fake.fields_of, fake.trace)
    assert [c for c in fake.calls if c[0] == "fields"] == [("fields", 0, 2), ("fields", 2, 3)]
    assert fake.buffers == [[2], [3]] and paths[0].shape == (3, 3) and count.tolist() == [1, 2, 3]


def test_all_counts_zero_give_one_column():
    fake = FakeSearch([0, 0, 0], 1)
    paths, count, _, _ = _grid.traced_search(3, "cpu", 1, 1, ((2,), (), ()), fake.fields_of, fake.trace)
    assert [tuple(t.shape) for t in paths] == [(3, 1, 2), (3, 1), (3, 1)] and count.tolist() == [0, 0, 0]
    assert not any(bool(t.any()) for t in paths)


def test_one_chunk_is_two_trace_calls():
    fake = FakeSearch([3, 7, 2, 7], 4)
    paths, count, _, _ = _grid.traced_search(4, "cpu", 4, 4, ((2,),), fake.fields_of, fake.trace)
    assert fake.calls == [("fields", 0, 4), ("size", 0), ("fill", 0)]
    assert paths[0].shape == (4, 7, 2) and count.tolist() == [3, 7, 2, 7]


@pytest.mark.parametrize("n_fields", [0, 3])
def test_an_empty_batch_traces_nothing(n_fields):
    fake = FakeSearch([], max(n_fields, 1))
    paths, count, status, cost = _grid.traced_search(0, "cpu", n_fields, 1, ((2,), (), ()), fake.fields_of, fake.trace)
    assert fake.calls == []
    assert [tuple(t.shape) for t in paths] == [(0, 1, 2), (0, 1), (0, 1)]
    assert count.shape == (0,) and status.shape == (0,) and cost.shape == (0, 2)
    assert all(t.dtype == torch.int32 for t in paths + [count, status, cost])


def test_every_goal_outside_is_one_sizing_pass_without_fields():
    fake = FakeSearch([5, 5], 1)
    paths, count, status, _ = _grid.traced_search(2, "cpu", 0, 1, ((2,),), fake.fields_of, fake.trace)
    assert fake.calls == [("size", 0)] and status.tolist() == [2, 2] and count.tolist() == [0, 0]
    assert paths[0].shape == (2, 1, 2) and not paths[0].any()


# ---- the frame -------------------------------------------------------------------------------------------------------------
BOUNDARIES, RES = (-0.3, 6.4, 0.2, 0.6), 0.1


def _frame_points():
    b = BOUNDARIES
    xs = [b[0] + k * RES for k in (0, 1, 64)] + [b[0] - 0.5 * RES, b[1] + 1.5 * RES, 3.14159, b[0] + 0.5 * RES]
    ys = [b[2] + k * RES for k in (0, 1, 64)] + [b[2] - 0.5 * RES, b[3] + 1.5 * RES, 0.41, b[2] + 3.5 * RES]
    return np.array([(x, y) for x in xs for y in ys], np.float64)


def test_cells_of_is_the_float64_floor_division_bit_for_bit():
    frame = _grid.GridFrame(BOUNDARIES, RES)
    pts = _frame_points()
    want = gsr.cells_of(pts, BOUNDARIES, RES)
    x_cells, y_cells = frame.cell_counts()
    assert (x_cells, y_cells) == (int((6.4 - -0.3) // 0.1) + 1, int((0.6 - 0.2) // 0.1) + 1)
    assert want[:, 1].min() == -1 and want[:, 1].max() >= x_cells and want[:, 0].min() == -1 and want[:, 0].max() >= y_cells
    for given in (pts, torch.from_numpy(pts), torch.from_numpy(np.concatenate([pts, np.ones((len(pts), 1))], 1))):
        got = frame.cells_of(given)
        assert got.dtype == torch.int32 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    # fp32 points are widened, not the arithmetic narrowed
    p32 = pts.astype(np.float32)
    assert np.array_equal(frame.cells_of(torch.from_numpy(p32)).numpy(), gsr.cells_of(p32, BOUNDARIES, RES))
    far = frame.cells_of(np.array([[1e30, -1e30], [-1e30, 1e30]]))
    assert far.tolist() == [[-2 ** 30, 2 ** 30], [2 ** 30, -2 ** 30]]


def test_cell_centres_are_the_reference_expression_bit_for_bit():
    frame = _grid.GridFrame(BOUNDARIES, RES)
    x, y, x_cells, y_cells = frame.cell_centres()
    assert (x_cells, y_cells) == frame.cell_counts() == (67, 4) and x.dtype == np.float64 and x.shape == y.shape == (67 * 4,)
    col, row = np.meshgrid(range(x_cells), range(y_cells))
    assert np.array_equal(x, col.reshape(-1) * RES + RES / 2 + BOUNDARIES[0])          # x fastest
    assert np.array_equal(y, row.reshape(-1) * RES + RES / 2 + BOUNDARIES[2])
    # every centre lies in its own cell
    cells = frame.cells_of(np.stack([x, y], 1)).numpy()
    assert np.array_equal(cells[:, 1], col.reshape(-1)) and np.array_equal(cells[:, 0], row.reshape(-1))
    assert frame.origin_resolution == (-0.3, 0.2, 0.1)
    assert _grid.cell_centres(BOUNDARIES, RES)[0].tobytes() == x.tobytes()


def test_what_a_frame_accepts_and_refuses():
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="resolution must be positive"):
            _grid.GridFrame(BOUNDARIES, bad)
    assert _grid.GridFrame((0, 1, 2), 1).boundaries == (0.0, 1.0, 2.0)        # OccupancyGrid's frame does not count them
    with pytest.raises(ValueError, match=r"boundaries must be \(x0, x1, y0, y1\)"):
        _grid.GridFrame((0, 1, 2), 1, four_sides=True)                          # LatticeGrid's does


def test_the_checker_chains():
    class Checker(object):
        pass
    bare, by_method, by_field = Checker(), Checker(), Checker()
    by_method.get_boundaries = lambda: [0, 1, 2, 3]
    by_method.boundaries = (9, 9, 9, 9)
    by_field.boundaries = (4, 5, 6, 7)
    assert _grid.checker_boundaries(by_method) == (0.0, 1.0, 2.0, 3.0) and _grid.checker_boundaries(by_field) == (4.0, 5.0, 6.0, 7.0)
    assert _grid.checker_boundaries(bare, (1, 2, 3, 4)) == (1.0, 2.0, 3.0, 4.0)
    with pytest.raises(ValueError, match="the checker carries no boundaries"):
        _grid.checker_boundaries(bare)
    assert _grid.checker_device(bare) == "cuda" and _grid.checker_device(bare, "cuda:1") == "cuda:1"
    by_field.obstacles = torch.zeros(1)
    assert _grid.checker_device(by_field) == torch.device("cpu")
    by_field.grid = Checker()
    by_field.grid.device = "cuda:2"
    assert _grid.checker_device(by_field) == "cuda:2" and _grid.checker_device(by_field, "cuda:0") == "cuda:0"


# ---- in front of a C entry -------------------------------------------------------------------------------------------------
def test_workspace_is_null_for_nothing_and_holds_what_was_asked():
    ws = _grid.workspace(0, "cpu")
    assert ws.ptr is None and ws.nbytes == 0
    for n in (1, 7, 8, 9):
        ws = _grid.workspace(n, "cpu")
        assert ws.nbytes == n and ws.buffer.numel() * ws.buffer.element_size() >= n and ws.ptr == ws.buffer.data_ptr()
        ctypes.memset(ws.ptr, 0xA5, n)                   # the pointer is the buffer's: all n bytes can be written
        assert ws.buffer.view(torch.uint8)[:n].tolist() == [0xA5] * n
    assert _grid.workspace(ctypes.c_size_t(16).value, "cpu").nbytes == 16


def test_int32_on_converts_and_keeps_what_is_already_right():
    right = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    a, b, c = _grid.int32_on("cpu", right, np.array([1.0, 2.0]), right.t())
    assert a.data_ptr() == right.data_ptr() and b.dtype == torch.int32 and b.tolist() == [1, 2]
    assert c.is_contiguous() and c.tolist() == right.t().tolist()
