"""The ppg_record_obs kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/obs_store_san_main.cpp: its own
`main`, the CPU wave emulator, buffers of exactly the stated sizes, a scalar reference; the capacity cut and a corrupted slot[t-1]
among its cases).  Nothing sanitised is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_obs_store_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "obs_store_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "obs_store_san_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OBS-STORE-SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
