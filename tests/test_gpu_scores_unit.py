"""The three update entry points of the skill scores share one kernel (k_metrics_partial<MISSING, TT, TP>, the member-aware form) and one
host function (metrics_update in rr_scores.hip).  Through the raw ABI: a single call and a members call of one member leave byte-equal
states, without and with skipped gaps, and member m's part of a three-member state is the single call on member m's rows, byte for byte."""
import numpy as np
import pytest

from river_route_amd import engine
from river_route_amd.engine import DeviceBuffer

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
S = engine.METRICS_STATE
# a chunk and a partial chunk of 32 rows; two column blocks of 256 and a ragged one
SHAPES = [(70, 300), (33, 7)]
M = 3


def split(n, rows, members=1):
    """metrics_split of rr_kernels_metrics.hpp, by hand: (splits, rows_per_split)."""
    col_blocks = members * -(-n // 256)
    chunks = -(-rows // 32)
    want = max(1, -(-2048 // col_blocks))
    splits = max(1, min(want, chunks))
    rows_per_split = -(-chunks // splits) * 32
    return max(1, -(-rows // rows_per_split)), rows_per_split


@pytest.fixture(scope='module')
def data():
    """Per shape: observations (rows, n) float64, the same with one NaN in the first row of the second chunk, and three members'
    simulations (M, rows, n) float64; left unchanged."""
    rng = np.random.default_rng(2027)
    out = {}
    for rows, n in SHAPES:
        obs = 5.0 + rng.gamma(2.0, 1.5, (rows, n))
        gapped = obs.copy()
        gapped[32, n // 2] = np.nan
        sim = np.stack([obs * rng.uniform(0.6, 1.4, n) + rng.normal(0.0, 0.5, (rows, n)) for _ in range(M)])
        for a in (obs, gapped, sim):
            a.setflags(write=False)
        out[rows, n] = obs, gapped, sim
    return out


def updated_state(members, rows, n, d_true, d_pred, pred_f32, missing, single=None):
    """The state one update leaves on zeros: `single` (an engine function) or the members call with `members` members and a shared
    observation block."""
    zeros = np.zeros(S * members * n)
    state = DeviceBuffer(zeros.nbytes).upload(zeros)
    if single is not None:
        work = DeviceBuffer(max(8, engine.metrics_work_bytes(n, rows)))
        single(n, rows, d_true, False, n, d_pred, pred_f32, n, None, state, work, work.nbytes)
    else:
        work = DeviceBuffer(max(8, engine.metrics_members_work_bytes(n, members, rows)))
        engine.metrics_update_members_dev(n, members, rows, d_true, False, n, 0, d_pred, pred_f32, n, rows * n, None, missing, state, work,
                                          work.nbytes)
    engine.synchronize(0)
    return state.download(F64, (S, members, n))


@pytest.mark.parametrize('pred_dtype', [F64, F32], ids=['pred_f64', 'pred_f32'])
@pytest.mark.parametrize('rows,n', SHAPES)
def test_single_calls_and_members_calls_leave_the_same_bytes(data, rows, n, pred_dtype):
    # rows <= 96: at most three chunks, fewer than the 2048 / (members x column blocks) splits wanted, so either call cuts the rows
    # into one split per 32-row chunk and a member's partial states meet the same row ranges in the same order
    assert split(n, rows) == split(n, rows, M) == (-(-rows // 32), 32)
    obs, gapped, sim = data[rows, n]
    sim = np.ascontiguousarray(sim.astype(pred_dtype))
    pred_f32 = pred_dtype == F32
    d_pred = DeviceBuffer(sim.nbytes).upload(sim)
    itemsize = sim.itemsize
    for missing, y_true, single in ((0, obs, engine.metrics_update_dev), (1, gapped, engine.metrics_update_missing_dev)):
        d_true = DeviceBuffer(y_true.nbytes).upload(y_true)
        alone = [updated_state(1, rows, n, d_true, d_pred.address + m * rows * n * itemsize, pred_f32, missing, single=single) for m in range(M)]
        assert alone[0][0].max() == rows and alone[0][0].min() == rows - missing       # the counts: the gap is skipped only when asked
        if not missing:
            assert not np.isnan(alone[0]).any()
        one = updated_state(1, rows, n, d_true, d_pred.address, pred_f32, missing)
        assert one.tobytes() == alone[0].tobytes(), f'members = 1, skip_missing = {missing}'
        three = updated_state(M, rows, n, d_true, d_pred.address, pred_f32, missing)
        for m in range(M):
            assert np.ascontiguousarray(three[:, m]).tobytes() == alone[m][:, 0].tobytes(), f'member {m} of {M}, skip_missing = {missing}'
