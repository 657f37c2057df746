"""Verify on upload (TSX_VERIFY) on the device: a failed chunk in the middle of a packed batch comes out the same - no bytes, no room, the
successor's offset - whether the waves wrote into the caller's buffer and the host packs in place, or the copies pack.  (Named to run
after the other GPU files.)"""
import pytest

from tests import verify_packed_cases as vp

pytestmark = pytest.mark.gpu


def test_a_failed_chunk_inside_a_packed_batch_packs_the_same_in_place_and_by_copies_on_the_device(gpu, oracle):
    assert vp.check_failed_chunk_in_packed_batch(gpu) == 32
