"""The ppg_net_forward / ppg_net_backward kernel source under AddressSanitizer and UBSan as a stand-alone program
(tests/net_san_main.cpp: its own `main`, the CPU wave emulator with four-wave workgroups, exactly the LDS of the HIP launch with the
bytes behind it poisoned, every tensor of exactly its stated size -- so a slot word that escaped its range check or a tap outside the
image would trap -- and a scalar float64 reference; the shapes of M around a tile and the invalid slots on the two smallest networks).
Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_net_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("net", "NET-SAN-CLEAN", tmp_path)
