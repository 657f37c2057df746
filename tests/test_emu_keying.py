"""Per-batch keys, AADs and IVs through every GCM path, on the CPU emulator (the bodies are tests/keying_cases.py; the device twins
are in tests/test_zzzzzzzzz_gpu_keying.py).  The emulator runs a launch to completion inside the call, so what it checks is the
arithmetic - AAD lengths 0 .. 64, the setup kernel against the host-built schedule, the tag check byte by byte - and the front end's
handling of the key between batches; a persistent kernel that outlives a batch's key exists on the device only."""
import pytest

from tests import keying_cases as kc


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_batch_kernels_under_a_fresh_key_aad_and_segment(emu, oracle, aad_len):
    kc.sweep_batch_kernels(emu, oracle, aad_len)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_setup_kernel_builds_the_schedule_the_host_builds(emu, oracle, aad_len):
    kc.sweep_setup_kernel(emu, oracle, aad_len)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_compressor_wave_encrypts_under_a_fresh_key_aad_and_segment(emu, oracle, aad_len):
    """Every frame size of 995 .. 1030 + 10 bytes without an AAD, with a partial AAD block and with the usual 32 bytes; at the other AAD
    lengths the sizes around the 63 / 64 / 65 block edges (a chunk costs the harness 0.1 s; the device test runs the whole range at
    every length)."""
    kc.sweep_fused(emu, oracle, aad_len, kc.FUSED_R_SIZES if aad_len in (0, 17, 32) else kc.FUSED_R_EDGES)


@pytest.mark.parametrize("aad_len", kc.AAD_LENGTHS)
def test_separate_launches_under_a_fresh_key_aad_and_segment(emu, oracle, aad_len):
    kc.sweep_separate(emu, oracle, aad_len)


def test_an_aad_of_65_bytes_is_refused(emu):
    kc.check_aad_len_65_is_refused(emu)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit_ctx", "pooled_ctx"])
def test_consecutive_batches_each_under_its_own_key(emu, oracle, explicit):
    """4 chunks of 16 KiB per batch here (16 of 256 KiB on the device)."""
    kc.check_consecutive_batches(emu, oracle, 16 << 10, explicit, nchunks=4)


def test_concurrent_members_each_under_their_own_key(emu, oracle):
    """4 threads x 6 batches x 2 chunks of 64 KiB (the harness compresses 0.1 MiB/s).  One caller at a time runs on it and a launch
    ends with its batch: the condition on shared launches is the device test's."""
    s0 = emu.service_stats(0)
    n = kc.check_concurrent_members(emu, oracle, threads=4, batches=6, chunk_size=64 << 10, nchunks=2)
    s1 = emu.service_stats(0)
    assert s1["members"] - s0["members"] >= n and s1["skipped_tickets"] == 0, (s0, s1)


def test_tamper_matrix(emu, oracle):
    assert kc.check_tamper_matrix(emu, oracle) == (2 * 23 + 2 * 25, 6)
