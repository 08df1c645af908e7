"""CPU: the sub-batch pipeline that the JPEG host path and the PNG decoder share (scannertools_amd/csrc/st_host_pipeline.h),
driven by scripts/host_pipeline_check.cpp under the sanitizers: a stand-alone program, never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scannertools_amd", "csrc")


def _build(cxx, exe, sanitize):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread"] + sanitize + ["-I" + CSRC, os.path.join(ROOT, "scripts", "host_pipeline_check.cpp"),
                           "-o", exe], capture_output=True, text=True)


@pytest.mark.parametrize("sanitize", [["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["thread", "address_undefined"])
def test_pipeline_check_is_clean_under_the_sanitizers(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_pipeline_check")
    res = _build(cxx, exe, sanitize)
    if res.returncode != 0:
        res = _build(cxx, exe, [])   # a toolchain without this sanitizer's runtime: the program's own assertions still run
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "WARNING: ThreadSanitizer" not in res.stderr, res.stdout[-2000:] + res.stderr[-4000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("host_pipeline_check: ") and last.endswith(" 0 failures") and int(last.split()[1]) >= 200


def test_the_header_includes_no_hip_and_the_decoders_hold_one_pipeline():
    """What makes the check above mean something: the decoders run the header's pipeline and have none of their own."""
    header = open(os.path.join(CSRC, "st_host_pipeline.h")).read()
    includes = [ln.split()[1] for ln in header.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "/" not in i and "." not in i for i in includes), includes   # the standard library only
    assert header.count("struct Shared") == 1
    for name in ("st_jpeg.hip", "st_png.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert "st_pipe_run(" in src and "struct Shared" not in src and "condition_variable" not in src, name
