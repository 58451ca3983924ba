"""The profiling instruments, the parts that need no GPU: the binding's tables against the text of include/avd.h.

  Context.KERNEL_IDS    is ``enum avd_kernel_id``: AVD_K_COUNT names, in the enum's order, under ONE naming rule --
                        drop ``AVD_K_``, lower-case, and write the enumerators that begin with FLOWUP as ``flow_up`` + size
                        (AVD_K_FLOWUP80 <-> flow_up80; every other name is the lower-cased enumerator as it stands).
  Context.stage_ms()    returns one value per stage the comment on avd_set_profiling documents (0 .. 5).
  the timing entries    avd_set_profiling, avd_stage_ms, avd_kernel_ms, avd_timer_start and avd_timer_stop are in the binding's symbol list and
                        exported by the built library.

The checker is shown to reject a permuted tuple and a tuple one entry short.  The instruments themselves are held to the header on the device
in tests/test_gpu_profiling.py."""
import inspect
import os
import re

import pytest

from avd_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING_SYMBOLS = ("avd_set_profiling", "avd_stage_ms", "avd_kernel_ms", "avd_timer_start", "avd_timer_stop")


def _header():
    with open(os.path.join(ROOT, "include", "avd.h")) as f:
        return f.read()


def _enum_kernel_ids(hdr):
    """the enumerators of ``enum avd_kernel_id`` in order, AVD_K_COUNT included; only the first may carry a value, and that value is 0"""
    body = re.search(r"enum avd_kernel_id \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for item in (t.strip() for t in body.split(",")):
        if not item:
            continue
        m = re.fullmatch(r"(AVD_K_\w+)(?:\s*=\s*(\d+))?", item)
        assert m, item
        assert m.group(2) is None or (not names and m.group(2) == "0"), item      # consecutive from 0: the position IS the value
        names.append(m.group(1))
    return names


def binding_name(enumerator):
    """the one rule: AVD_K_<NAME> -> name, with FLOWUP<size> written flow_up<size>"""
    assert enumerator.startswith("AVD_K_")
    return re.sub(r"^flowup(?=\d)", "flow_up", enumerator[len("AVD_K_"):].lower())


def check_kernel_ids(ids, hdr):
    """-> list of differences between a KERNEL_IDS tuple and the header's enum (empty: they agree)"""
    enum = _enum_kernel_ids(hdr)
    if enum[-1] != "AVD_K_COUNT":
        return ["AVD_K_COUNT is not the last enumerator"]
    want = [binding_name(e) for e in enum[:-1]]
    bad = []
    if len(ids) != len(want):
        bad.append(f"{len(ids)} names for AVD_K_COUNT = {len(want)}")
    bad += [f"id {i}: binding {a!r}, header {b!r}" for i, (a, b) in enumerate(zip(ids, want)) if a != b]
    return bad


def documented_stages(hdr):
    """the stage numbers the comment on avd_set_profiling describes: every ``<digit> = `` of that comment"""
    comment = re.findall(r"/\*((?:(?!\*/).)*)\*/\s*int avd_set_profiling\(", hdr, re.S)
    assert len(comment) == 1
    return [int(d) for d in re.findall(r"(?<![\w.])(\d) = ", comment[0])]


def test_kernel_ids_are_the_headers_enum():
    hdr = _header()
    enum = _enum_kernel_ids(hdr)
    assert len(enum) == 16 and enum[0] == "AVD_K_PREPROCESS" and enum[-1] == "AVD_K_COUNT"
    assert len(set(enum)) == len(enum)
    assert check_kernel_ids(_lib.Context.KERNEL_IDS, hdr) == []
    assert binding_name("AVD_K_FLOWUP80") == "flow_up80" and binding_name("AVD_K_LEVEL320") == "level320"
    # kernel_ms() asks the library for position i under name i: the tuple is what it iterates
    src = inspect.getsource(_lib.Context.kernel_ms)
    assert "enumerate(self.KERNEL_IDS)" in src and "avd_kernel_ms(self._h, i," in src


@pytest.mark.parametrize("control", ["permuted", "one-short"])
def test_the_checker_rejects_a_wrong_tuple(control):
    hdr = _header()
    ids = list(_lib.Context.KERNEL_IDS)
    if control == "permuted":
        i, j = ids.index("stats"), ids.index("records")
        ids[i], ids[j] = ids[j], ids[i]
    else:
        ids = ids[:-1]
    bad = check_kernel_ids(tuple(ids), hdr)
    assert bad, control
    assert len(bad) == (2 if control == "permuted" else 1), bad


def test_stage_ms_returns_the_documented_stages():
    stages = documented_stages(_header())
    assert stages == [0, 1, 2, 3, 4, 5], stages
    m = re.search(r"for i in range\((\d+)\):", inspect.getsource(_lib.Context.stage_ms))
    assert m and int(m.group(1)) == len(stages)


def test_the_timing_entry_points_are_bound_and_exported():
    _lib.build()
    L = _lib.load()
    hdr = _header()
    declared = set(re.findall(r"^\s*int\s+(avd_\w+)\s*\(", hdr, re.M))
    for name in TIMING_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name                       # dlsym on the built library
        assert getattr(L, name).argtypes is not None, name
    assert len(L.avd_kernel_ms.argtypes) == len(L.avd_stage_ms.argtypes) == 3
    assert len(L.avd_timer_start.argtypes) == 1 and len(L.avd_timer_stop.argtypes) == 2 and len(L.avd_set_profiling.argtypes) == 2
