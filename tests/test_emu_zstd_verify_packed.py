"""Verify on upload (TSX_VERIFY) under the CPU emulator: a failed chunk in the middle of a packed batch comes out the same - no bytes, no
room, the successor's offset - whether the waves wrote into the caller's buffer and the host packs in place, or the copies pack."""
from tests import verify_packed_cases as vp


def test_a_failed_chunk_inside_a_packed_batch_packs_the_same_in_place_and_by_copies(emu, oracle):
    assert vp.check_failed_chunk_in_packed_batch(emu) == 32
