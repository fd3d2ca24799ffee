"""The ppg_record_logp kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/logp_san_main.cpp: its own
`main`, the CPU wave emulator, buffers of exactly the stated sizes, a scalar reference; the capacity cut, corrupted slot words,
out-of-range actions, A = 32 and rows of -inf among its cases).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_logp_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("logp", "LOGP-SAN-CLEAN", tmp_path)
