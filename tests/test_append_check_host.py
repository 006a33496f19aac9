"""The host-side checks of the append entries (csrc/append_check.cpp: attention_append's and kv_rows_append's refusal functions, the
latent stream's argument validation) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/append_check_main.cpp, a
stand-alone program with its own main, is compiled together with that file and run on the CPU.  No GPU, no Python extension, no
preloaded runtime; the program's exit status and the sanitizers' reports are the verdict."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "index-tts-ipex_amd", "csrc")


def test_append_checks_under_host_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "append_check_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "host", "append_check_main.cpp"),
           os.path.join(CSRC, "append_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-4000:], ran.stderr[-4000:])
    assert "every case answered as expected" in ran.stdout
