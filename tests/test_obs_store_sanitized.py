"""The ppg_record_obs kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/obs_store_san_main.cpp: its own
`main`, the CPU wave emulator, buffers of exactly the stated sizes, a scalar reference; the capacity cut and a corrupted slot[t-1]
among its cases).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_obs_store_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("obs_store", "OBS-STORE-SAN-CLEAN", tmp_path)
