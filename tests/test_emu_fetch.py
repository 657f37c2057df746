"""The fetch side in a broker's shapes under the CPU emulator (tests/fetch_cases.py): damaged frames with valid tags behind the GCM stage,
mixed verdicts through the piece pipeline up to 65 chunks, segment-sized slots, one context and the pool from batch to batch.  The
emulator runs streams in order: what it shows is slices, copies and carried state, not missing waits - those are the device file's."""
import pytest

from tests import fetch_cases as fc


def test_corpus_and_batches_meet_their_conditions(oracle):
    """Conditions on libzstd, OpenSSL and the plans alone."""
    fc.cc.need157(oracle)
    fc.check_corpus(oracle)
    fc.check_pieces_rule()
    for n in fc.SHAPES:
        for caps in ("exact", "segment"):
            fc.check_plan(oracle, fc.make_plan(oracle, n, caps, "contiguous", small=n >= 256, rot=n))
    fc.sequence_plans(oracle)


SHAPES = [(15, "segment", "contiguous", "pageable"), (16, "exact", "padded", "registered"), (16, "segment", "contiguous", "device"),
          (17, "segment", "padded", "pageable"), (17, "exact", "contiguous", "device"), (33, "segment", "contiguous", "registered"),
          (65, "segment", "contiguous", "pageable")]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n,caps,layout,mem", SHAPES)
def test_mixed_verdicts_in_every_cut(emu, oracle, n, caps, layout, mem):
    fc.cc.need157(oracle)
    fc.check_shapes(emu, oracle, n, caps, layout, mem)


@pytest.mark.timeout(900)
def test_mixed_verdicts_under_the_flags_word_of_the_java_layer(emu, oracle):
    fc.cc.need157(oracle)
    fc.check_shapes(emu, oracle, 33, "segment", "contiguous", "pageable", flags=fc.JAVA)


@pytest.mark.timeout(900)
def test_pieces_one_piece_and_chunk_form_each_match_the_reference(emu, oracle):
    fc.cc.need157(oracle)
    fc.check_forms_and_cuts(emu, oracle)


@pytest.mark.timeout(900)
def test_one_context_through_five_fetches_of_other_shapes(emu, oracle):
    fc.cc.need157(oracle)
    fc.check_one_context_in_sequence(emu, oracle)


@pytest.mark.timeout(900)
def test_four_pooled_callers_of_other_shapes_at_once(emu, oracle):
    fc.cc.need157(oracle)
    fc.check_pooled_callers(emu, oracle)
