"""Every frame feature libzstd 1.5.7 emits and the whole damaged corpus of tests/frame_vocab_cases.py through both decoder forms of the
product library, where tests/test_emu_frame_vocab.py can afford the vocabulary and a third of the corpus; plus frames of full chunk
size on either side of the block form's limit of 264 blocks.  tests/test_emu_frames_asan.py has had the same frames under
AddressSanitizer on the CPU.  (Named to run after the other GPU files.)"""
import pytest

from tests import frame_vocab_cases as fv
from tests import zstd_inspect as zi

pytestmark = pytest.mark.gpu
_FULL = None


def full_size_cases(o):
    """Record batches ("B") at level 3 with a target block size of 16 KiB: 4 MiB, and two sizes whose frames have just under and just
    over 264 blocks.  -> [(name, source, frame)]"""
    global _FULL
    if _FULL is None:
        big = fv.B(5350000)
        _FULL = [(name, big[:n].tobytes(), fv.libzstd_frame(o, big[:n], [(fv.LEVEL, 3), (fv.TARGET_CBLOCK, 16384)]))
                 for name, n in (("B 4 MiB", 4 << 20), ("B just under 264 blocks", 5300000), ("B just over 264 blocks", 5350000))]
    return _FULL


def test_full_size_frames_lie_on_both_sides_of_the_block_limit(oracle):
    """Conditions on libzstd's frames alone."""
    fv.cc.need157(oracle)
    blocks = [len(zi.parse_frame(f, decode=False)[1]) for _, _, f in full_size_cases(oracle)]
    print(blocks, [len(f) for _, _, f in full_size_cases(oracle)])
    assert blocks[0] <= fv.ZB_MAX_BLOCKS and fv.ZB_MAX_BLOCKS - 8 <= blocks[1] <= fv.ZB_MAX_BLOCKS < blocks[2] <= fv.ZB_MAX_BLOCKS + 8, blocks
    assert all(len(f) < 4500000 for _, _, f in full_size_cases(oracle))


def test_both_forms_restore_the_vocabulary_on_the_device(gpu, oracle):
    fv.cc.need157(oracle)
    fv.check_vocabulary_is_covered(oracle)
    fv.check_both_forms_restore(gpu, oracle, extra=full_size_cases(oracle))


def test_both_forms_share_libzstd_verdict_on_damage_on_the_device(gpu, oracle):
    fv.cc.need157(oracle)
    fv.check_the_corpus_is_balanced(oracle)
    classes = fv.check_verdicts(gpu, oracle)
    assert classes["both accept"] >= 100 and classes["both reject"] >= 100, classes
    good = fv.vocabulary(oracle)[0]                                      # the device still works afterwards
    res = fv.decode_batches(gpu, [good[2]], [len(good[1])])
    assert res["block"][1] == [0] and res["block"][0] == [good[1]]
