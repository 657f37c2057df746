"""Both decoder forms under the CPU emulator over every frame feature libzstd 1.5.7 emits, and held to libzstd's own verdict on
damaged frames (tests/frame_vocab_cases.py).  The whole damaged corpus runs on the device; here every third frame of it does, which
keeps every kind of region in."""
import pytest

from tests import frame_vocab_cases as fv


def subset(o):
    return [i for i in range(len(fv.damaged(o))) if i % 3 == 0]


def test_libzstd_frames_hold_the_whole_vocabulary(oracle):
    fv.cc.need157(oracle)
    fv.check_vocabulary_is_covered(oracle)


def test_damaged_corpus_splits_between_both_verdicts_and_covers_every_region(oracle):
    fv.cc.need157(oracle)
    fv.check_the_corpus_is_balanced(oracle)
    D = fv.damaged(oracle)
    assert {D[i].kind for i in subset(oracle)} == set(fv.KINDS)


@pytest.mark.timeout(900)
def test_both_forms_restore_the_vocabulary(emu, oracle):
    fv.cc.need157(oracle)
    fv.check_vocabulary_is_covered(oracle)
    fv.check_both_forms_restore(emu, oracle)


@pytest.mark.timeout(900)
def test_both_forms_share_libzstd_verdict_on_damage(emu, oracle):
    fv.cc.need157(oracle)
    classes = fv.check_verdicts(emu, oracle, subset(oracle))
    assert classes["both accept"] >= 20 and classes["both reject"] >= 20, classes
