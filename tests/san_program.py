"""TEST-ONLY: builds and runs one of the stand-alone sanitizer programs (tests/<name>_san_main.cpp: its own `main`, the CPU wave
emulator, a scalar reference) under AddressSanitizer and UBSan.  Nothing sanitised is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_clean(name, marker, tmp_path):
    exe = tmp_path / f"{name}_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", f"{name}_san_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and marker in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
