"""The call table and the comparison of tests/test_gpu_history.py, checked without a GPU: the table names every ingest / analysis entry point
of the C-ABI, and the comparison that referees the histories rejects what it has to reject."""
import numpy as np

import avd_hip
from tests import history_calls as T


def test_the_table_covers_every_declared_entry_point():
    """a new avd_preprocess_* / avd_analyze_* entry point cannot be added to the header without joining the table"""
    declared = T.declared_entry_points()
    assert {"avd_preprocess_bgr", "avd_farneback_pairs", "avd_analyze_pictures_async", "avd_analyze_frame_lists"} <= declared
    covered = set().union(*(e.symbols for e in T.TABLE))
    assert covered == declared, covered ^ declared
    assert all(e.symbols and e.kind in ("pre", "fb", "rec") for e in T.TABLE)
    assert all(hasattr(avd_hip._lib.load(), s) for s in covered)


def test_the_table_is_tiny_and_its_other_content_has_the_same_shapes():
    def arrays(x):
        if isinstance(x, np.ndarray):
            return [x]
        if isinstance(x, avd_hip.Pixels):
            return arrays(x.data)
        if isinstance(x, (tuple, list)):
            return [a for v in x for a in arrays(v)]
        return []
    for e in T.TABLE:
        a, b = arrays(e.inputs()), arrays(T.other_content(e.inputs()))
        assert a and [(v.shape, v.dtype) for v in a] == [(v.shape, v.dtype) for v in b], e.name
        assert all(not np.array_equal(v, w) for v, w in zip(a, b)), e.name
        assert sum(v.nbytes for v in a) <= 6 * 320 * 320 * 3, e.name
    assert T.table_geometries() == [(67, 101), (48, 64), (45, 832), (34, 48), (45, 64), (96, 128), (64, 48), (33, 40)]
    assert T.fb_frames().shape == (4, 320, 320) and T.clip96().shape == (5, 96, 128, 3)
    assert np.array_equal(T.clip96()[1], T.clip96()[2]) and not np.array_equal(T.clip96()[2], T.clip96()[3])
    assert len(T.big_clip()) - 1 > 128                      # grows the Farneback scratch past what it holds at first


def _result():
    rec = np.zeros(3, avd_hip.RECORD_DTYPE)
    rec["lap_sum"], rec["lap_sumsq"], rec["flow_mean"], rec["flow_var"], rec["ham"] = [5, -6, 7], [50, 60, 70], [0, 0.5, 1.5], [0, 2.5, 3.5], [-1, 3, 4]
    return {"records": rec, "rerun_pairs": np.zeros(1, np.int32), "area": np.arange(3 * 1024, dtype=np.uint8).reshape(3, 32, 32),
            "flow0": np.array([[0.0, -0.0, np.nan, 1.0]], np.float32), "poly3": np.ones((3, 40, 40, 5), np.float32)}


def test_the_comparison_accepts_a_copy():
    assert T.differences({k: v.copy() for k, v in _result().items()}, _result()) == []


def test_the_comparison_rejects_one_changed_byte_in_every_field():
    want = _result()
    for field in avd_hip.RECORD_DTYPE.names:               # `reserved` included
        for row in range(3):
            got = {k: v.copy() for k, v in want.items()}
            got["records"][field][row:row + 1].view(np.uint8)[0] ^= 1
            bad = T.differences(got, want)
            assert len(bad) == 1 and bad[0].startswith("records: 1 of 96 bytes differ"), (field, row, bad)
    for name in want:
        got = {k: v.copy() for k, v in want.items()}
        got[name].reshape(-1).view(np.uint8)[-1] ^= 0x80
        bad = T.differences(got, want)
        assert len(bad) == 1 and bad[0].startswith(f"{name}: 1 of "), (name, bad)


def test_the_comparison_counts_nan_payloads_and_the_sign_of_zero():
    want = _result()
    got = {k: v.copy() for k, v in want.items()}
    assert T.differences(got, want) == []                  # NaN equals the same NaN: bytes are compared, not values
    got["flow0"][0, 0] = -0.0
    assert T.differences(got, want) == ["flow0: 1 of 16 bytes differ, the first at byte 3 (element 0)"]
    got = {k: v.copy() for k, v in want.items()}
    got["flow0"].view(np.uint32)[0, 2] ^= 1                 # another NaN
    assert np.isnan(got["flow0"][0, 2]) and len(T.differences(got, want)) == 1


def test_the_comparison_rejects_a_missing_an_extra_and_a_reshaped_buffer():
    want = _result()
    for name in want:
        got = {k: v.copy() for k, v in want.items() if k != name}
        assert T.differences(got, want) == [f"{name}: missing"]
    got = dict(want, pyr0=np.zeros(4, np.float32))
    assert T.differences(got, want) == ["pyr0: not in the reference"]
    got = dict(want, area=want["area"][:2])
    assert len(T.differences(got, want)) == 1
    got = dict(want, area=want["area"].astype(np.int8))
    assert len(T.differences(got, want)) == 1
