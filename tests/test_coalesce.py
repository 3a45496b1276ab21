"""The chunk coalescer's planning logic (misonet_amd/coalesce.py) against a fake runner: no GPU."""
import pytest

from misonet_amd.coalesce import Item, coalesce


class FakeRunner:
    """records every batch; a row's output is its (item, b, split) tag, so the test can check where each chunk went"""

    def __init__(self):
        self.batches, self.in_flight, self.max_in_flight, self.log = [], 0, 0, []

    def submit(self, i, chunks):
        assert i == len(self.batches)
        self.batches.append([(c.item.index, c.b, c.split) for c in chunks])
        self.in_flight += 1
        self.max_in_flight = max(self.max_in_flight, self.in_flight)
        self.log.append(("submit", i))
        return i

    def collect(self, i):
        self.in_flight -= 1
        self.log.append(("collect", i))
        return [("row", i, r, tag) for r, tag in enumerate(self.batches[i])]


def _items(spec):
    """spec: list of (n_b, n_split, T)"""
    return [Item(i, b, k, T, payload=f"item{i}") for i, (b, k, T) in enumerate(spec)]


def _run(spec, max_batch, depth=2):
    r = FakeRunner()
    done = list(coalesce(iter(_items(spec)), r.submit, r.collect, max_batch, depth))
    return r, done


def _check_outputs(done, spec):
    assert [it.index for it in done] == list(range(len(spec)))              # loader order
    for it in done:
        assert it.missing == 0
        for k in range(it.n_split):
            for b in range(it.n_b):
                assert it.outputs[k][b][3] == (it.index, b, k)


def test_full_batches_and_short_last():
    spec = [(1, 1 + i % 3, 48) for i in range(12)]                          # 24 chunks
    r, done = _run(spec, 5)
    sizes = [len(b) for b in r.batches]
    assert sizes == [5, 5, 5, 5, 4]
    _check_outputs(done, spec)
    # every chunk exactly once, in loader order, split-major within an item
    flat = [t for b in r.batches for t in b]
    assert flat == [(i, 0, k) for i, (_, n, _) in enumerate(spec) for k in range(n)]


def test_three_split_item_straddles_a_boundary():
    spec = [(1, 1, 48), (1, 3, 48), (1, 2, 48)]                             # item 1's splits land in two batches
    r, done = _run(spec, 2)
    assert r.batches == [[(0, 0, 0), (1, 0, 0)], [(1, 0, 1), (1, 0, 2)], [(2, 0, 0), (2, 0, 1)]]
    _check_outputs(done, spec)
    r, done = _run(spec, 3)
    assert r.batches == [[(0, 0, 0), (1, 0, 0), (1, 0, 1)], [(1, 0, 2), (2, 0, 0), (2, 0, 1)]]
    _check_outputs(done, spec)


def test_items_with_two_utterances():
    spec = [(2, 2, 48), (2, 1, 48), (1, 3, 48)]
    r, done = _run(spec, 4)
    assert r.batches[0] == [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)]    # split-major: the per-item row order
    assert r.batches[1] == [(1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1)]
    assert r.batches[2] == [(2, 0, 2)]
    _check_outputs(done, spec)


def test_shape_change_flushes():
    spec = [(1, 2, 48), (1, 1, 48), (1, 2, 64), (1, 1, 64), (1, 1, 48)]
    r, done = _run(spec, 16)
    assert [len(b) for b in r.batches] == [3, 3, 1]
    assert {t[0] for t in r.batches[0]} == {0, 1} and {t[0] for t in r.batches[1]} == {2, 3}
    _check_outputs(done, spec)


def test_max_batch_one_and_empty_loader():
    spec = [(1, 3, 48), (2, 1, 48), (1, 1, 48)]
    r, done = _run(spec, 1)
    assert [len(b) for b in r.batches] == [1] * 6
    _check_outputs(done, spec)
    r, done = _run([], 16)
    assert done == [] and r.batches == []
    with pytest.raises(ValueError):
        list(coalesce(iter(_items(spec)), r.submit, r.collect, 0))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_in_flight_bounded_by_depth_and_completion_in_order(depth):
    spec = [(1 + i % 2, 1 + i % 3, 48) for i in range(20)]
    r = FakeRunner()
    seen = []
    for it in coalesce(iter(_items(spec)), r.submit, r.collect, 4, depth):
        seen.append(it.index)
        # an item is handed out only once every batch holding one of its chunks has been collected
        collected = {i for op, i in r.log if op == "collect"}
        assert all(bi in collected for bi, b in enumerate(r.batches) for t in b if t[0] == it.index)
    assert seen == list(range(len(spec)))
    assert r.max_in_flight <= depth
    assert r.max_in_flight == min(depth, len(r.batches))
    assert r.in_flight == 0


def test_loader_read_ahead_is_bounded():
    """the loader is read lazily: while the first items are handed out, at most max_batch pending chunks plus the
    batches in flight have been read"""
    read = []
    max_batch, depth = 4, 2

    def loader():
        for i in range(1000):
            read.append(i)
            yield Item(i, 1, 1 + i % 3, 48)

    r = FakeRunner()
    for it in coalesce(loader(), r.submit, r.collect, max_batch, depth):
        chunks_read = sum(1 + i % 3 for i in read)
        chunks_done = sum(1 + i % 3 for i in range(it.index + 1))
        assert chunks_read - chunks_done <= max_batch * (depth + 1) + 3
        if it.index == 50:
            break
    assert len(read) < 70


def test_runner_row_count_is_checked():
    spec = [(1, 2, 48)]
    with pytest.raises(RuntimeError):
        list(coalesce(iter(_items(spec)), lambda i, c: i, lambda h: [], 2))
