"""The hand-scheduled edge pair loop of the trimmed dataflow item on the GPU
(k_iter_flow<double, vvo2_t, 0, 1>; gqmap_tuning.h GQ_EDGE_SCHED,
gqmap_math.h edge_sums_range_sched).

The item's own edge jobs, its halo chain slices and the grouped bottom-row
items all run one pair loop, which reads a pair's XI / XJ a pair ahead (row
k + 1 beside pair k's weights, the centre point from the last read-ahead) and
takes a pair's two roots side by side.  The same operations on the same
operands, so every bit must be what it was: state, trace and MAP flow against
the CPU model (oracle.emu_run) and against one launch per iteration.

The crops and starts of tests/test_gpu_item_trim.py, whose runs are shared
(one run per case in a session, left unchanged): 40 x 56 -- full 16 x 16
tiles, a right column of 8 node columns -- and 36 x 40, whose last tile row of
4 node rows runs as grouped items beside chain items.  K = 9, and K = 2 and 3,
whose chains have empty and one-pair slices (2 and 4 mirror pairs: the
read-ahead of an empty slice is the row of its first pair that is not there,
K = 3's last one the centre's), at 12 iterations from the seeded start and
from means on the flow range's ends.  Then the stop rule firing inside a
launch, and a frame outside the tap table's range, which takes the pair
store's kernel with the unscheduled loop.
"""
import numpy as np
import pytest

from tests.test_gpu_item_trim import ITS, KS, _cpu, _ref, _run, _same, _start, _vs_cpu_model
from tests.test_gpu_tap_lut import CROPS, _opts

pytestmark = pytest.mark.gpu


def test_cases_cover_empty_and_one_pair_slices():
    """chain_cut at GQ_FLOW_HALO_EPI = 8 (gqmap_math.h): K = 2 cuts its two
    pairs into one slice of two and three empty ones, K = 3 its four into
    slices of three and of one pair and two empty ones (the last of them
    takes the centre point); K = 9 has none of either."""
    def cut(K):
        n = K * K // 2
        c = [min(n, (n + 8) * w // 4) for w in range(5)]
        return [b - a for a, b in zip(c, c[1:])]
    assert KS == [9, 2, 3]
    assert cut(2) == [2, 0, 0, 0] and cut(3) == [3, 1, 0, 0] and cut(9) == [12, 12, 12, 4]


@pytest.mark.parametrize("start", ["seeded", "edges"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_scheduled_loop_bit_exact_vs_cpu_model(rows, cols, K, start):
    got = _ref(rows, cols, K, "flow", start)
    assert got[4] == 1  # the offset store: the kernel with the scheduled loop
    _vs_cpu_model(got, _cpu(rows, cols, K, start))


@pytest.mark.parametrize("start", ["seeded", "edges"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_scheduled_loop_bit_exact_vs_per_launch(rows, cols, K, start):
    a, b = _ref(rows, cols, K, "launch", start), _ref(rows, cols, K, "flow", start)
    assert a[0] == ITS and b[0] == ITS and b[4] == 1
    _same(a, b)


def test_stop_rule_inside_the_launch():
    """tor just above a value of sum|dmu| that lies below every earlier one:
    finalize(k) stops the run while items of iteration k + 1 are in flight,
    their pair loops included; rows, state and MAP flow as one launch per
    iteration leaves them."""
    rows, cols, its = 40, 56, 40
    o = _opts(rows, cols, 9)
    seed = _start(rows, cols, 9, "seeded")
    _, tr0, *_ = _run(rows, cols, o, its, "launch", seed)
    warm = int(np.argmax(tr0[:its - 8, 1])) + 1  # sum|dmu| first climbs from the seeded state: start past its peak
    start = _run(rows, cols, o, warm, "launch", seed)[2]
    its -= warm
    _, tr, *_ = _run(rows, cols, o, its, "launch", start)
    run_min = np.minimum.accumulate(tr[:, 1])
    ks = [k for k in range(2, its) if tr[k, 1] < run_min[k - 1]]
    assert ks, f"no new minimum of sum|dmu| in rows [2, {its}): {tr[:, 1]}"
    k = ks[len(ks) // 2]
    tor = float(tr[k, 1]) * (1 + 1e-12)
    assert int(np.argmax(tr[:, 1] < tor)) == k and k + 1 < its
    o = _opts(rows, cols, 9, tor=tor)
    a = _run(rows, cols, o, its, "launch", start)
    b = _run(rows, cols, o, its, "flow", start)
    assert b[4] == 1 and a[0] == b[0] == k + 1
    _same(a, b)


@pytest.mark.parametrize("K", [9, 3])
def test_frame_beyond_the_table_keeps_the_pair_store_kernel(K):
    rows, cols = CROPS[0]
    got = _ref(rows, cols, K, "flow", "seeded", "wide")
    assert got[4] == 0
    _vs_cpu_model(got, _cpu(rows, cols, K, "seeded", "wide"))
    _same(_ref(rows, cols, K, "launch", "seeded", "wide"), got)
