"""The ppg_backward_samples kernel source under AddressSanitizer and UBSan as a stand-alone program
(tests/backward_samples_san_main.cpp: its own `main`, the CPU wave emulator, exactly the LDS of the HIP launch with the bytes behind it
poisoned, every tensor of exactly its stated size -- so a slot word that escaped its range check would trap -- and a scalar
reference).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_backward_samples_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("backward_samples", "BACKWARD-SAMPLES-SAN-CLEAN", tmp_path)
