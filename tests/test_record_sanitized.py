"""The ppg_record kernel source (with the link it calls) under AddressSanitizer and UBSan as a stand-alone program
(tests/record_san_main.cpp: its own `main`, the CPU wave emulator, exactly the LDS of the HIP launch with the bytes behind it
poisoned, buffers of exactly [T,B,S] elements, a scalar reference).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_record_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("record", "RECORD-SAN-CLEAN", tmp_path)
