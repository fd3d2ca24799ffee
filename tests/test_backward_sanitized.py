"""The ppg_backward kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/backward_san_main.cpp: its own
`main`, the CPU wave emulator, exactly the LDS of the HIP launch with the bytes behind it poisoned, tensors of exactly [T,B,S]
elements, a scalar reference).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_backward_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("backward", "BACKWARD-SAN-CLEAN", tmp_path)
