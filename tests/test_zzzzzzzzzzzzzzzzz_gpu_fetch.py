"""The fetch side in a broker's shapes on the device (tests/fetch_cases.py; tests/test_emu_fetch.py has run the same bodies on the CPU
emulator up to 65 chunks): damaged frames with valid tags behind the GCM stage and mixed verdicts through every cut of the piece
pipeline - where pieces really run side by side on four compute streams and two copy-out streams - up to 256 chunks and the chunk form's
257, segment-sized slots back to back, one context and the pool from batch to batch.  (Named to run after the other GPU files.)"""
import pytest

from tests import fetch_cases as fc
from tests import test_emu_fetch as emu_tests

pytestmark = pytest.mark.gpu


def test_corpus_and_batches_meet_their_conditions(oracle):
    emu_tests.test_corpus_and_batches_meet_their_conditions(oracle)


# every size in both cap rules, both layouts and the three kinds of memory at least once; the cut sizes in all three kinds of memory
SHAPES = emu_tests.SHAPES + [(15, "exact", "padded", "device"), (16, "segment", "contiguous", "pageable"), (17, "segment", "contiguous", "registered"),
                             (33, "segment", "padded", "device"), (33, "exact", "contiguous", "pageable"), (65, "exact", "padded", "registered"),
                             (65, "segment", "contiguous", "device"),
                             (256, "segment", "contiguous", "pageable"), (256, "segment", "contiguous", "registered"), (256, "exact", "padded", "device"),
                             (256, "exact", "contiguous", "registered"), (257, "segment", "contiguous", "pageable"), (257, "exact", "padded", "registered"),
                             (257, "segment", "contiguous", "device")]


@pytest.mark.parametrize("n,caps,layout,mem", SHAPES)
def test_mixed_verdicts_in_every_cut(gpu, oracle, n, caps, layout, mem):
    emu_tests.test_mixed_verdicts_in_every_cut(gpu, oracle, n, caps, layout, mem)


@pytest.mark.parametrize("n", [33, 256])
def test_mixed_verdicts_under_the_flags_word_of_the_java_layer(gpu, oracle, n):
    fc.cc.need157(oracle)
    fc.check_shapes(gpu, oracle, n, "segment", "contiguous", "registered", flags=fc.JAVA)


def test_pieces_one_piece_and_chunk_form_each_match_the_reference(gpu, oracle):
    emu_tests.test_pieces_one_piece_and_chunk_form_each_match_the_reference(gpu, oracle)


def test_one_context_through_five_fetches_of_other_shapes(gpu, oracle):
    emu_tests.test_one_context_through_five_fetches_of_other_shapes(gpu, oracle)


def test_four_pooled_callers_of_other_shapes_at_once(gpu, oracle):
    emu_tests.test_four_pooled_callers_of_other_shapes_at_once(gpu, oracle)
