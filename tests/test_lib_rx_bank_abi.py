"""The entry points of the two banks of extra receivers on the paths that need no device (tests/rx_bank_abi_harness.cpp): a null
ctx, a count over the maximum, a null list with a nonzero count come back as SSDR_EINVAL from both families.  No GPU.  (The same
program compiled together with the library's sources under -fsanitize=address,undefined is the host code's sanitizer check: its
header has the command.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_before_any_device_work_return_their_codes(tmp_path):
    from supersdr_amd import _lib as L
    exe = str(tmp_path / "rx_bank_abi_harness")
    lib_dir = os.path.dirname(os.path.abspath(L.LIB_PATH))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "rx_bank_abi_harness.cpp"),
                           L.LIB_PATH, "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASS" in out.stdout, out.stdout + out.stderr
