"""The repeat-offset history on the device: the cases of tests/test_emu_decoder_stages.py against the product library, where the
history lives in scalar registers and the lane exchanges are real.  (Named to run after the other GPU files.)"""
import pytest

from tests import decoder_stage_cases as ds

pytestmark = pytest.mark.gpu


def test_both_forms_restore_the_chunk_on_the_device(gpu, oracle):
    ds.check_the_input_exercises_the_history(oracle)
    ds.check_both_forms_restore_the_chunk(gpu, oracle)


def test_both_forms_agree_on_a_damaged_frame_on_the_device(gpu, oracle):
    ds.check_both_forms_agree_on_damage(gpu, oracle)
