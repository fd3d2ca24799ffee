"""The repack map and the word function of ppg_policy_update under AddressSanitizer and UBSan as a stand-alone program
(tests/policy_update_san_main.cpp: its own `main`, only the HIP-free header csrc/ppg_policy_pack.h, every parameter tensor and the image
a heap block of exactly its size -- so a map entry whose index leaves its tensor would trap -- over the shapes of
tests/policy_update_cases.py, compared byte for byte with the image of ppg_policy_fragments_of).  Nothing sanitised is loaded into
python."""
from tests.san_program import assert_clean


def test_policy_update_map_and_word_function_are_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("policy_update", "POLICY-UPDATE-SAN-CLEAN", tmp_path)
