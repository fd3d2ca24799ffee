"""The plan of ppg_policy_evaluate under AddressSanitizer and UBSan as a stand-alone program (tests/policy_evaluate_san_main.cpp: its
own `main`, only the HIP-free header csrc/ppg_policy_plan.h -- the inline functions the kernel ppg_policy_plan_rows calls -- with the
plan a heap block of exactly the reported size, over tile mode and range mode, slots {1, 3, 512}, capacities {1, 200, 70000} and the
count list of tests/test_policy_evaluate_plan.py, checked against a scalar restatement).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_policy_evaluate_plan_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("policy_evaluate", "POLICY-EVALUATE-SAN-CLEAN", tmp_path)
