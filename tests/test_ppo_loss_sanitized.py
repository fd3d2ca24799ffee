"""The ppg_ppo_loss kernel source under AddressSanitizer and UBSan as a stand-alone program (tests/ppo_loss_san_main.cpp: its own
`main`, the CPU wave emulator, exactly the LDS of the HIP launch with the bytes behind it poisoned, every tensor of exactly its stated
size -- so a slot word or an action that escaped its range check would trap -- and a scalar reference; the invalid-sample kinds and
the chunk-edge shapes).  Nothing sanitised is loaded into python."""
from tests.san_program import assert_clean


def test_ppo_loss_kernel_source_is_clean_under_asan_and_ubsan(tmp_path):
    assert_clean("ppo_loss", "PPO-LOSS-SAN-CLEAN", tmp_path)
