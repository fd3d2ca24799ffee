"""The ppg_record_logp kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/logp_san_main.cpp: its own
`main`, the CPU wave emulator, buffers of exactly the stated sizes, a scalar reference; the capacity cut, corrupted slot words,
out-of-range actions, A = 32 and rows of -inf among its cases).  Nothing sanitised is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_logp_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "logp_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "logp_san_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "LOGP-SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
