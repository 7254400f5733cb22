"""How `HelperJobBatcher` (janus_amd/multijob.py) packs aggregation jobs into GPU batches and maps
a task's batch slots to aggregate slots.  CPU only: no engine call."""
import numpy as np
import pytest

from janus_amd.multijob import aggregate_slots, pack_jobs


def _check(sizes, max_reports, batches):
    """The contract, whatever the sizes: order kept, no job split or repeated, zeros in no batch,
    every batch within the bound unless it is one oversize job."""
    flat = [j for b in batches for j in b]
    assert flat == [j for j, n in enumerate(sizes) if n > 0]
    for b in batches:
        assert b
        total = sum(sizes[j] for j in b)
        assert total <= max_reports or len(b) == 1
    # greedy: a batch was closed only because the next job did not fit
    for b, nb in zip(batches, batches[1:]):
        assert sum(sizes[j] for j in b) + sizes[nb[0]] > max_reports


def test_order_kept_and_no_job_split():
    sizes = [1, 3, 8, 13, 64, 65, 2, 7, 20, 5, 4]
    got = pack_jobs(sizes, 70)
    assert got == [[0, 1, 2, 3], [4], [5, 6], [7, 8, 9, 10]]
    _check(sizes, 70, got)
    assert pack_jobs(sizes, 65536) == [list(range(len(sizes)))]


def test_oversize_job_alone():
    sizes = [10, 500, 10, 10]
    got = pack_jobs(sizes, 100)
    assert got == [[0], [1], [2, 3]]
    _check(sizes, 100, got)
    assert pack_jobs([500], 100) == [[0]]
    assert pack_jobs([500, 600], 100) == [[0], [1]]


def test_zeros_skipped():
    sizes = [0, 5, 0, 0, 5, 0]
    assert pack_jobs(sizes, 10) == [[1, 4]]
    assert pack_jobs(sizes, 9) == [[1], [4]]
    assert pack_jobs([0, 0], 10) == []


def test_exact_fits():
    assert pack_jobs([50, 50, 50, 50], 100) == [[0, 1], [2, 3]]
    assert pack_jobs([100, 100], 100) == [[0], [1]]
    assert pack_jobs([99, 1, 1], 100) == [[0, 1], [2]]
    assert pack_jobs([1] * 7, 3) == [[0, 1, 2], [3, 4, 5], [6]]


def test_empty_list():
    assert pack_jobs([], 100) == []


def test_random_lists_keep_the_contract():
    rng = np.random.default_rng(11)
    for _ in range(200):
        sizes = [int(x) for x in rng.choice([0, 1, 2, 63, 64, 65, 100, 500, 1000],
                                            size=rng.integers(0, 30))]
        mx = int(rng.choice([1, 64, 100, 512, 65536]))
        _check(sizes, mx, pack_jobs(sizes, mx))


def test_bad_bound():
    with pytest.raises(ValueError):
        pack_jobs([1], 0)


def test_slots_per_task():
    assert aggregate_slots(0, 2, np.array([0, 1, 1], np.uint64)).tolist() == [0, 1, 1]
    got = aggregate_slots(3, 2, np.array([1, 0], np.uint64))
    assert got.dtype == np.uint32 and got.tolist() == [7, 6]
    assert aggregate_slots(5, 1, np.zeros(0, np.uint32)).tolist() == []
    with pytest.raises(ValueError, match="slot 2"):
        aggregate_slots(1, 2, np.array([0, 2], np.uint64))  # would land in task 2's slots
    with pytest.raises(ValueError):
        aggregate_slots(0, 1, np.array([1], np.uint32))
    with pytest.raises(ValueError):
        aggregate_slots(0, 4, np.array([-1], np.int64))
