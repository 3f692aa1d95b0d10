"""Every header of csrc stands alone: a file that includes nothing but that header passes the
device syntax check, so each header includes what it names and no include order is implied.
(gm_fphelpers.inc is a fragment its includers expand twice on purpose, not a header.)"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gripper-mujoco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (gm_newton.hip is a stage header in all but its suffix: the physics stages include it)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + ["gm_newton.hip"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not installed")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    src = tmp_path / "one.hip"
    src.write_text(f'#include "{header}"\n')
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17",
                        "-I" + os.path.join(REPO, "include"), "-I" + CSRC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
