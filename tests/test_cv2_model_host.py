"""Option "cv2_model" without a GPU: the header's text, the binding's constants against the oracle's, the unchanged symbol set, and
tools/pick_cv2_model.py on golden files this test writes itself (the generator's keys, the oracle's flows in the role of cv2's)."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import avd_hip
from avd_hip import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_documents_the_option():
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    at = hdr.index('"cv2_model" (default 0')
    text = hdr[at:hdr.index('"audio_format" (0 float32', at)]
    assert "AVD_CV2_MODEL" in text and 'begins "cv2_model:"' in text
    for bit, name in ((1, "GAUSS_MULADD"), (8, "THREE_SCALES"), (16, "RESIZE_LERP")):
        assert re.search(rf"^ \*\s+{bit}\s+{name}\b", text, re.M), name
    # the three consequences of bit 8
    assert "AVD_K_LEVEL40 and AVD_K_FLOWUP80 are exactly 0" in text
    assert "still tile stage 2" in text
    assert re.search(r"bits 3 and 7 of\s+\*?\s*avd_frame_record\.reserved are never set", text)
    assert '"fb_model" int32[4]' in hdr


def test_constants_equal_the_oracles(oracle):
    assert avd_hip.CV2_GAUSS_MULADD == oracle.MODEL_GAUSS_MULADD == 1
    assert avd_hip.CV2_THREE_SCALES == oracle.MODEL_THREE_SCALES == 8
    assert avd_hip.CV2_RESIZE_LERP == oracle.MODEL_RESIZE_LERP == 16
    src = open(os.path.join(ROOT, "oracle", "avd_oracle.h")).read()
    for name, value in (("GAUSS_MULADD", 1), ("THREE_SCALES", 8), ("RESIZE_LERP", 16)):
        assert re.search(rf"AVDO_MODEL_{name}\s*=\s*{value}\b", src), name
    internal = open(os.path.join(ROOT, "ai-video-detector_amd", "csrc", "avd_internal.h")).read()
    assert re.search(r"kCv2GaussMuladd = 1, kCv2ThreeScales = 8, kCv2ResizeLerp = 16\b", internal)


def test_the_exported_symbol_set_is_unchanged():
    """an option, never a function: 43 + 3 exports, ABI 3"""
    assert len(_lib.EXPORTS) == 43 and len(_lib.LIST_EXPORTS) == 3
    nm = shutil.which("nm")
    assert nm, "no nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.build()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T avd_\w+$", line)}
    assert exported == set(_lib.EXPORTS) | set(_lib.LIST_EXPORTS), exported ^ (set(_lib.EXPORTS) | set(_lib.LIST_EXPORTS))
    assert _lib.load().avd_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "avd.h")).read()
    assert "AVD_K_COUNT" in hdr and len(_lib.Context.KERNEL_IDS) == 15          # no avd_kernel_id was added


@pytest.fixture(scope="module")
def picker():
    spec = importlib.util.spec_from_file_location("pick_cv2_model", os.path.join(ROOT, "tools", "pick_cv2_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden_under_9(oracle):
    """the generator's keys for two small clips: one with the dense flow, one with the statistics only; the "cv2" is the oracle under mask 9"""
    data = {"info": np.frombuffer(b'{"cv2": "oracle under mask 9"}', np.uint8)}
    for (n, h, w, seed), dense in (((3, 96, 128, 0), True), ((3, 72, 96, 5), False)):
        small = oracle.preprocess_bgr(synth.make_clip(n, h, w, seed=seed, dup_every=0))[0]
        with oracle.model(9):
            flows = np.stack([oracle.farneback(small[p], small[p + 1]) for p in range(n - 1)])
        st = [oracle.flow_stats(f) for f in flows]
        key = f"{h}x{w}"
        data[key + "/small320"] = small
        data[key + "/flow_mean"] = np.array([s[0] for s in st], np.float32)
        data[key + "/flow_var"] = np.array([s[1] for s in st], np.float32)
        if dense:
            data[key + "/flow"] = flows
    return data


def test_picker_names_the_mask(picker, golden_under_9, oracle, tmp_path, capsys):
    path = str(tmp_path / "cv2_stage_golden.npz")
    np.savez(path, **golden_under_9)
    assert picker.main([path]) == 0
    out = capsys.readouterr().out
    assert re.search(r"^AVD_CV2_MODEL=9\b", out, re.M), out
    with np.load(path) as z:
        rows = picker.evaluate(z, oracle)
    assert picker.pick(rows) == 9
    assert rows[9]["pairs"] == 4 and rows[9]["identical"] == 4 and rows[9]["max_diff"] == 0.0
    for mask in picker.MASKS:
        if mask != 9:
            assert rows[mask]["identical"] < rows[mask]["pairs"], mask           # no other mask reproduces every pair
    assert oracle.lib().avdo_get_model() == 0                                   # the tool leaves the oracle as it found it


def test_picker_reports_a_pair_no_mask_reproduces(picker, golden_under_9, tmp_path, capsys):
    data = dict(golden_under_9)
    flows = data["96x128/flow"].copy()
    v = flows[1].reshape(-1).view(np.uint32)
    v[12345] += 1                                                             # one ulp in one component of one pixel
    data["96x128/flow"] = flows
    path = str(tmp_path / "cv2_stage_golden.npz")
    np.savez(path, **data)
    assert picker.main([path]) == 1
    out = capsys.readouterr().out
    assert "no mask matches" in out and "AVD_CV2_MODEL=" not in out, out
    row9 = next(line for line in out.splitlines() if re.match(r"\s*9\s", line))
    assert "96x128[1] (flow:" in row9 and "96x128[0]" not in row9, row9         # that pair, and under mask 9 only that pair
    assert re.search(r"closest: 9\b", out), out
