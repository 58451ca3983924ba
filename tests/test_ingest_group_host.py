"""Option "ingest_group" without a GPU: the plan (csrc/avd_ingest_group.h), the header's text (include/avd.h) and avd_hip.StreamMux(group=...).

tests/ingest_group_check.cpp is a stand-alone program (tests/ingest_group_kit.py compiles it with AddressSanitizer and UBSan and RUNS it; nothing
is loaded into Python).  Without arguments it enumerates every call of up to four clips with a key out of three, n in {0, 1, 2, 5}, output
frames with and without gaps, under the library's bound and under one that splits groups -- (1 + 12 + 12^2 + 12^3 + 12^4) x 2 x 2 = 90 484
calls -- and runs the same checker over two planners that break the rule on purpose; with "key:n:f0" arguments it prints one call's plan.
"""
import os
import re

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib

from tests import ingest_group_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV12 = _lib.AVD_FMT_NV12


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_is_plain_host_code():
    text = open(kit.HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") or i == '"avd_ingest_clip.h"' for i in includes) and not [i for i in includes if "hip" in i], includes
    assert "constexpr int64_t kMaxLaunchBands" in text


def test_every_call_of_up_to_four_clips_and_the_two_controls():
    status, out = kit.run()
    m = re.fullmatch(r"ingest groups: 90484 calls checked, 0 failures; control without row_stride rejected in (\d+) calls, control without gaps in (\d+)\n", out)
    assert status == 0 and m, (status, out)
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0


def test_interleaved_keys():
    # positions 0, 2, 5 share key 0; 1 has the padded rows; 3, 4 are NV12; a clip without frames is nowhere
    groups, total = kit.plan((0, 2, 0), (1, 1, 2), (0, 5, 3), (2, 1, 8), (2, 2, 9), (0, 1, 11), (1, 0, 12))
    assert [g["members"] for g in groups] == [[0, 2, 5], [1], [3, 4]]
    assert [g["grouped"] for g in groups] == [1, 0, 1]
    assert groups[0]["out"] == [0, 1, 3, 4, 5, 6, 7, 11] and groups[1]["out"] == [2] and groups[2]["out"] == [8, 9, 10]
    # the runs of row partials [frames][h][32] and Laplacian partials [frames][nbands][8][2]: group after group
    row = [g["frames"] * kit.KEY_H[k] * 32 for g, k in zip(groups, (0, 1, 2))]
    lap = [g["frames"] * kit.KEY_NBANDS[k] * kit.LAP_SLOTS * 2 for g, k in zip(groups, (0, 1, 2))]
    assert [g["rowbuf"] for g in groups] == [0, row[0], row[0] + row[1]] and total[0] == sum(row)
    assert [g["lappart"] for g in groups] == [0, lap[0], lap[0] + lap[1]] and total[1] == sum(lap)


def test_the_stream_map_shape_has_gaps():
    # eight one-frame streams, each behind its carry frame: output frames 1, 3, ..., 15 in ONE group
    groups, _ = kit.plan(*[(2, 1, 2 * i + 1) for i in range(8)])
    assert len(groups) == 1 and groups[0]["grouped"] == 1 and groups[0]["out"] == list(range(1, 16, 2))


def test_no_shared_key_is_the_per_clip_call():
    groups, _ = kit.plan((0, 3, 0), (1, 3, 3), (2, 3, 6))
    assert [g["members"] for g in groups] == [[0], [1], [2]] and not any(g["grouped"] for g in groups)


def test_a_group_is_split_at_the_bound():
    # five bands a frame, at most 30 bands a launch: 5 + 1 frames fit, the third clip opens a new group, which the fourth joins
    groups, _ = kit.plan((0, 5, 0), (0, 1, 5), (0, 2, 6), (0, 2, 8), bound=30)
    assert [g["members"] for g in groups] == [[0, 1], [2, 3]]
    # a clip that alone passes the bound is alone, as it is without the option
    groups, _ = kit.plan((0, 5, 0), (0, 5, 5), bound=20)
    assert [g["members"] for g in groups] == [[0], [1]] and not any(g["grouped"] for g in groups)


@pytest.mark.parametrize("bad", ["x", "3:1:0", "1:2"])
def test_dump_mode_refuses_what_it_cannot_read(bad):
    status, _ = kit.run(bad)
    assert status == 2


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def _flat(block):
    return re.sub(r"\s*\n \*\s*", " ", block)


def _comment_before(text, decl):
    end = text.index(decl)
    return _flat(text[text.rindex("/*", 0, end):end])


def test_header_has_a_paragraph_for_the_option():
    text = open(os.path.join(ROOT, "include", "avd.h")).read()
    flat = _comment_before(text, "int avd_set_option(")
    at = flat.index('"ingest_group" (default 0')
    assert at > flat.index('"stream_map":')
    rest = flat[at:flat.index('"audio_format" (0 float32', at)]
    assert "0 or 1" in rest and "AVD_ERR_ARG" in rest and 'begins "ingest_group:"' in rest and "durable" in rest
    for part in ("height and width", "layout", "rotate", "full range", "row strides", "16-byte fills"):
        assert part in rest, part
    assert "ONE ingest launch and ONE k_hash launch per group" in rest
    assert "A group of ONE clip runs today's per-clip path" in rest
    assert "avd_preprocess_*" in rest and "bit for bit" in rest
    assert "Left out as well" not in flat
    fetch = _comment_before(text, "int64_t avd_debug_fetch(")
    assert '"ingest_call" int32[4]' in fetch and '"ingest_groups" int32[launches][4]' in fetch and "{live clips, live clips, 0, 0}" in fetch
    assert re.search(r"#define\s+AVD_ABI_VERSION\s+3\b", text) and len(_lib.EXPORTS) == 43 and "ingest_group(" not in text


def test_the_library_has_the_option_row():
    text = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_capi.hip")).read()
    assert re.search(r'\{"ingest_group", &avd_ctx::ingest_group, true, opt_ingest_group,', text)
    assert "static bool opt_ingest_group(int& v) { return v == 0 || v == 1; }" in text       # 2 and -1 are refused (on the GPU: tests/test_gpu_ingest_group.py)
    internal = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_internal.h")).read()
    assert re.search(r"// option \"ingest_group\":.*\n(\s*//.*\n)*\s*int ingest_group = 0;", internal)


# ---- StreamMux --------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """what StreamMux needs of a Context; every call is appended to .calls.  It refuses option values as the library does."""

    def __init__(self, group=0):
        self.calls, self.pending, self.options = [], None, {"ingest_group": group}

    def stream_reset(self, slot=0):
        self.calls.append(("reset", slot))

    def stream_map(self, mapping=None):
        self.calls.append(("map", dict(mapping or {})))

    def get_option(self, name):
        self.calls.append(("get", name))
        return self.options[name]

    def set_option(self, name, value):
        self.calls.append(("set", name, value))
        if name == "ingest_group" and value not in (0, 1):
            raise _lib.AvdError("avd status -1: ingest_group: 0 (an ingest and a hash launch per clip) or 1")
        self.options[name] = value

    def analyze_frame_lists_async(self, lists, rec, rotates=None, full_ranges=None):
        assert self.pending is None
        self.calls.append(("async", self.options["ingest_group"]))
        self.pending = rec
        return None

    def synchronize(self):
        self.calls.append(("sync",))
        self.pending = None


def surfaces(n, h=4, w=6):
    return [(np.full((h, w), i, np.uint8), np.full((h // 2, w), 128, np.uint8)) for i in range(n)]


def test_the_recorder_refuses_2_and_minus_1_and_keeps_the_old_value():
    r = Recorder(group=1)
    for bad in (2, -1):
        with pytest.raises(_lib.AvdError, match="ingest_group:"):
            r.set_option("ingest_group", bad)
    assert r.options["ingest_group"] == 1


def test_group_none_makes_no_extra_call():
    r = Recorder()
    out = avd_hip.StreamMux(ctx=r, chunk=2).run([(surfaces(3), NV12), (surfaces(2), NV12)])
    assert [len(o) for o in out] == [3, 2]
    assert [c[0] for c in r.calls] == ["reset", "reset", "map", "async", "sync", "async", "sync", "sync", "map"]
    assert not [c for c in r.calls if c[0] in ("get", "set")]


@pytest.mark.parametrize("was,group", [(0, True), (1, False), (1, True)])
def test_group_sets_the_option_and_restores_it(was, group):
    r = Recorder(group=was)
    avd_hip.StreamMux(ctx=r, chunk=2, group=group).run([(surfaces(3), NV12), (surfaces(2), NV12)])
    names = [c[0] for c in r.calls]
    assert names == ["reset", "reset", "map", "get", "set", "async", "sync", "async", "sync", "sync", "set", "map"]
    assert r.calls[4] == ("set", "ingest_group", int(group)) and r.calls[-2] == ("set", "ingest_group", was)
    assert [c[1] for c in r.calls if c[0] == "async"] == [int(group)] * 2      # every round ran under the asked value
    assert r.options["ingest_group"] == was


def test_the_option_is_restored_after_an_exception_and_after_the_drain():
    def broken():
        yield from surfaces(2)
        raise OSError("decoder failed")

    r = Recorder(group=0)
    with pytest.raises(OSError, match="decoder failed"):
        avd_hip.StreamMux(ctx=r, chunk=2, group=True).run([(surfaces(4), NV12), (broken(), NV12)])
    assert [c[0] for c in r.calls] == ["reset", "reset", "map", "get", "set", "async", "sync", "set", "map"]
    assert r.options["ingest_group"] == 0 and r.pending is None
