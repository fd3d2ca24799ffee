"""The ppg_backward_samples kernel source under AddressSanitizer and UBSan as a stand-alone program
(tests/backward_samples_san_main.cpp: its own `main`, the CPU wave emulator, exactly the LDS of the HIP launch with the bytes behind it
poisoned, every tensor of exactly its stated size -- so a slot word that escaped its range check would trap -- and a scalar
reference).  Nothing sanitised is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_samples_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "backward_samples_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "backward_samples_san_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "BACKWARD-SAMPLES-SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
