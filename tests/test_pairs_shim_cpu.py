"""The preload shim's paired-end session (BMH_PAIRS_SAM_DEVICE=1) without a GPU: the refusal when the library is loaded, that the
single-end switch's refusal is still its own, and the pipeline tool's flag."""
import os
import subprocess
import sys

import pytest

import kswlib
from __graft_entry__ import load_package

MESSAGE = b"[bwamem_hip] fatal: BMH_PAIRS_SAM_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n"
CODE = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"


def _load(env_more):
    """the shim loaded into a child interpreter behind the reference library, as test_reads_sam_shim_cpu.py loads it"""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    env = dict(os.environ)
    for k in ("BMH_REGS_DEVICE", "BMH_MATESW_DEVICE", "BMH_WANTED_DEVICE", "BMH_PHASE2_DEVICE", "BMH_PHASE2_TEXT_DEVICE", "BMH_REGION_LONG", "BMH_READS_SAM_DEVICE",
              "BMH_PAIRS_SAM_DEVICE", "BMH_PAC_RESIDENT"):
        env.pop(k, None)
    env.update(env_more)
    return subprocess.run([sys.executable, "-c", CODE, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)


def test_shim_refuses_the_switch_without_resident_reference_at_load():
    """BMH_PAIRS_SAM_DEVICE=1 with BMH_PAC_RESIDENT=0: status 1 and the sibling's message under the new name, before any GPU work"""
    r = _load({"BMH_PAIRS_SAM_DEVICE": "1", "BMH_PAC_RESIDENT": "0"})
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert MESSAGE in r.stderr and b"loaded" not in r.stdout
    assert b"BMH_READS_SAM_DEVICE" not in r.stderr


def test_shim_loads_with_the_switch_otherwise():
    for more in ({"BMH_PAIRS_SAM_DEVICE": "1"}, {"BMH_PAIRS_SAM_DEVICE": "0", "BMH_PAC_RESIDENT": "0"}, {"BMH_PAIRS_SAM_DEVICE": "1", "BMH_PAC_RESIDENT": "1"}):
        r = _load(more)
        assert r.returncode == 0 and b"loaded" in r.stdout, (more, r.stderr.decode()[-500:])


def test_pipeline_tool_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(kswlib.ROOT, "tools", "pipeline_bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--pairs-sam-device" in r.stdout and "BMH_PAIRS_SAM_DEVICE=1" in r.stdout
    assert "--reads-sam-device" in r.stdout  # the sibling's flag stays
