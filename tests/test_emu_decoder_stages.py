"""The repeat-offset history under the CPU emulator: libzstd's level-3 and level-19 frames of one chunk, counted first (every history
index in use, users at the start of later blocks, blocks of more than 64 sequences), then decoded by the block form and by the chunk
form, which resolve the history through the same function (csrc/zstd_dec_dev.h, dec_rep_offsets).  The device twin is
tests/test_zzzzzzzzzz_gpu_decoder_stages.py."""
from tests import decoder_stage_cases as ds


def test_the_frames_use_every_entry_of_the_history(oracle):
    ds.check_the_input_exercises_the_history(oracle)


def test_both_forms_restore_the_chunk(emu, oracle):
    ds.check_the_input_exercises_the_history(oracle)
    ds.check_both_forms_restore_the_chunk(emu, oracle)


def test_both_forms_agree_on_a_damaged_frame(emu, oracle):
    ds.check_both_forms_agree_on_damage(emu, oracle)
