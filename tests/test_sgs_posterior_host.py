"""Host check of sgs.batch_plan: the batch sizes of the small-scale drivers (and, on steps, of run_many_pcg64) when a posterior
snapshot has to end a batch.  No device."""
import numpy as np
import pytest

from mcmc_gpu_amd import posterior, sgs

N_ITERS = (1, 31, 32, 33, 61, 120)
BATCHES = (1, 32, 128)
SCHEDULES = (None, (0, 1), (0, 7), (11, 5), (0, 40), (59, 1))       # (burn_in, thin)


def _todays_sizes(n_iter, batch):
    """what the drivers did before there were snapshots: min(batch, remaining) until nothing remains"""
    sizes, done = [], 0
    while done < n_iter:
        sizes.append(min(batch, n_iter - done))
        done += sizes[-1]
    return sizes


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n_iter", N_ITERS)
def test_batch_plan(n_iter, batch, schedule):
    its = None if schedule is None else posterior.snapshot_iterations(n_iter, *schedule)
    sizes = sgs.batch_plan(n_iter, batch, its)
    assert all(isinstance(k, int) and 1 <= k <= batch for k in sizes), sizes
    assert sum(sizes) == n_iter
    ends = set(int(e) - 1 for e in np.cumsum(sizes))             # the last iteration of every batch
    if its is not None:
        assert set(int(k) for k in its) <= ends, (sizes, its)
        # no cut that neither a snapshot nor a full batch asks for: a batch is short only where a snapshot or the run ends it
        start = 0
        for k in sizes:
            assert k == batch or start + k - 1 in set(int(v) for v in its) or start + k == n_iter, (sizes, its)
            start += k
    if its is None or its.size == 0:
        assert sizes == _todays_sizes(n_iter, batch)


def test_batch_plan_cases_cover_the_edges():
    """The schedules above contain a snapshot at iteration 0, one at n_iter - 1, a thin above the batch and one dividing it."""
    assert posterior.snapshot_iterations(61, 0, 7)[0] == 0 and posterior.snapshot_iterations(61, 0, 1)[-1] == 60
    assert posterior.snapshot_iterations(120, 59, 1)[-1] == 119
    assert sgs.batch_plan(120, 32, posterior.snapshot_iterations(120, 0, 40)) == [1, 32, 8, 32, 8, 32, 7]      # thin above the batch
    assert sgs.batch_plan(33, 32, posterior.snapshot_iterations(33, 0, 1)) == [1] * 33                         # thin dividing it
    assert sgs.batch_plan(61, 32, [0, 7, 60]) == [1, 7, 32, 21]
    assert sgs.batch_plan(61, 32, None) == [32, 29] == sgs.batch_plan(61, 32, [])
    assert sgs.batch_plan(33, 32, [31]) == [32, 1] and sgs.batch_plan(33, 32, [32]) == [32, 1]
    assert sgs.batch_plan(5, 128, [7, -1]) == [5]               # iterations outside the run cut nothing


def test_batch_plan_refuses_nonsense():
    with pytest.raises(ValueError):
        sgs.batch_plan(0, 32)
    with pytest.raises(ValueError):
        sgs.batch_plan(10, 0)
