"""librr_hip.so is built from two device translation units (rr_engine.hip: routing; rr_scores.hip: skill scores and overlap areas) that
share one error string: rr_last_error names the latest refusal of the calling thread, whichever unit refused."""
import ctypes as C
import threading

from river_route_amd import _lib
from river_route_amd._lib import RR_E_INVALID


def test_last_error_is_one_string_for_both_units_and_per_thread():
    L, out = _lib.lib(), C.c_int64(0)

    def last():
        return L.rr_last_error().decode()

    scores_unit = 'rr_metrics_work_bytes: sizes out of range'
    assert L.rr_metrics_work_bytes(-1, 1, C.byref(out)) == RR_E_INVALID and last() == scores_unit
    assert L.rr_dev_alloc_stats(None) == RR_E_INVALID and last() == 'rr_dev_alloc_stats: null out'          # the routing unit
    assert L.rr_metrics_work_bytes(-1, 1, C.byref(out)) == RR_E_INVALID and last() == scores_unit
    assert L.rr_plan_info(None, None) == RR_E_INVALID and last() == 'rr_plan_info: null argument'
    assert L.rr_metrics_work_bytes(-1, 1, C.byref(out)) == RR_E_INVALID and last() == scores_unit

    seen = []

    def other_thread():
        mine = C.c_int64(0)
        seen.append(last())                                                  # a fresh thread has no refusal yet
        seen.append((L.rr_plan_info(None, None), last()))
        seen.append((L.rr_metrics_adjoint_work_bytes(-1, C.byref(mine)), last()))

    t = threading.Thread(target=other_thread)
    t.start()
    t.join()
    assert seen == ['', (RR_E_INVALID, 'rr_plan_info: null argument'), (RR_E_INVALID, 'rr_metrics_adjoint_work_bytes: sizes out of range')]
    assert last() == scores_unit                                             # this thread's string is as it was
