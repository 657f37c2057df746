"""Per-batch keys, AADs and IVs through every GCM path, on the device (the bodies are tests/keying_cases.py).  What only the device can
show: compressor waves of a live service kernel read the key schedule, the AAD and the IVs from pinned host memory that the host
rewrites for every batch and wipes after it, with no kernel boundary between one batch's key and the next.  Every batch here has a
key, AAD and segment of its own and every expectation is OpenSSL's, so a stale or cross-member read gives wrong bytes.  (Named to run
after the other GPU files.)"""
import pytest

import tsxform
from tests import keying_cases as kc

nat = tsxform._native
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_batch_kernels_under_a_fresh_key_aad_and_segment_on_the_device(gpu, oracle, aad_len):
    kc.sweep_batch_kernels(gpu, oracle, aad_len)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_setup_kernel_builds_the_schedule_the_host_builds_on_the_device(gpu, oracle, aad_len):
    kc.sweep_setup_kernel(gpu, oracle, aad_len)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_compressor_wave_encrypts_under_a_fresh_key_aad_and_segment_on_the_device(gpu, oracle, aad_len):
    kc.sweep_fused(gpu, oracle, aad_len)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_separate_launches_under_a_fresh_key_aad_and_segment_on_the_device(gpu, oracle, aad_len):
    kc.sweep_separate(gpu, oracle, aad_len)


def test_final_kernel_lane_loop_wraps_with_a_17_byte_aad(gpu, oracle):
    """62 and 64 sub-blocks of 64 KiB and a byte: 63 and 65 partial GHASH values plus the AAD and the length item are 65 and 67 items
    for gcm_final_kernel's 64 lanes - lane 0 (then lanes 0 .. 2) takes a second item, the AAD and length items change lanes."""
    (key, aad, seg), rng = kc.sweep_params(17)
    chunks = kc.rand_chunks(rng, [62 * 65536 + 1, 64 * 65536 + 1])
    kc.check_keyed(gpu, oracle, nat.ENCRYPT, chunks, key, aad, seg, "final kernel wrap")


def test_an_aad_of_65_bytes_is_refused_on_the_device(gpu):
    kc.check_aad_len_65_is_refused(gpu)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit_ctx", "pooled_ctx"])
def test_consecutive_batches_each_under_its_own_key_on_the_device(gpu, oracle, explicit):
    kc.check_consecutive_batches(gpu, oracle, 256 << 10, explicit)


def test_concurrent_members_each_under_their_own_key_on_the_device(gpu, oracle):
    """8 threads x 6 batches x 16 chunks of 256 KiB, every batch under its own key.  The condition that keeps the test honest: the 48
    compressing batches were members of FEWER than 48 launches of the service kernel, so batches with different keys shared a live
    kernel - waves went from one member's key to another's without a kernel boundary between them.  (A 16-chunk host batch goes as two
    members, so 96 or more are expected; a 256 KiB chunk keeps its wave busy for tens of milliseconds against the kernel's 2 ms idle
    exit, so a handful of launches is expected.  The counts the test prints have not been recorded from a device run yet; should
    the condition on launches not hold in this shape, the shape changes - more threads, or svc_idle_exit_us raised - not the assertion.)"""
    gpu.service_quiesce(0)
    s0 = gpu.service_stats(0)
    n = kc.check_concurrent_members(gpu, oracle, threads=8, batches=6, chunk_size=256 << 10)
    gpu.service_quiesce(0)
    s1 = gpu.service_stats(0)
    members, launches = s1["members"] - s0["members"], s1["launches"] - s0["launches"]
    print("%d compressing batches under %d keys: %d members in %d launches of the service kernel" % (n, n, members, launches))
    assert members >= n, (s0, s1)
    assert 1 <= launches < n, (s0, s1)
    assert s1["skipped_tickets"] == 0, (s0, s1)
    assert gpu.pool_stats(0)["in_use"] == 0


def test_tamper_matrix_on_the_device(gpu, oracle):
    assert kc.check_tamper_matrix(gpu, oracle) == (2 * 23 + 2 * 25, 6)
