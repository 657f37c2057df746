/*
 * JNI binding of libtsxform's C ABI (include/tsxform.h).  One native method per entry point the hot path needs;
 * java/jni/tsx_jni.c is the shim.  NOT compiled in this repository's CI (no JDK in the build image) - see INTEGRATION.md.
 */
package io.aiven.kafka.tieredstorage.gpu;

import java.nio.ByteBuffer;

public final class TsxNative {
    public static final int COMPRESS = 0x1;
    public static final int ENCRYPT = 0x2;
    public static final int CRC = 0x4;
    /**
     * With {@link #COMPRESS} on transform: every frame carries a Zstandard content checksum ({@code compression.zstd.checksum}; libzstd's
     * ZSTD_c_checksumFlag, byte for byte).  The flags travel through {@link #transformBatch} and its siblings as they are.  Detransform
     * needs no flag: a frame that declares a checksum is always verified, a mismatch is {@link #E_BAD_FRAME}.
     */
    public static final int ZSTD_CHECKSUM = 0x8;
    /**
     * With {@link #COMPRESS} on transform: verify on upload ({@code compression.zstd.verify}).  Every frame the device has written is read
     * back and compared with its chunk before the chunk is reported; a chunk whose frame does not restore it has status
     * {@link #E_VERIFY}.  Detransform accepts and ignores the flag.
     */
    public static final int VERIFY = 0x20;
    /**
     * With {@link #ENCRYPT} on transform: verify on upload, AES-GCM stage ({@code encryption.verify}).  The IV || C || TAG the device has
     * delivered for a chunk is decrypted and authenticated on the device, against the bytes the stage was given, before the chunk is
     * reported; a chunk that fails has status {@link #E_VERIFY}.  Without {@link #ENCRYPT} the batch is refused; detransform accepts and
     * ignores the flag.
     */
    public static final int VERIFY_GCM = 0x80;
    /**
     * On transform, with any chain: validate the source ({@code segment.records.validate}).  The batch's chunks, in order, are ONE stream
     * that begins and ends on a record-batch boundary - a whole log segment; every v2 record batch of it is checked on the device (length,
     * magic, CRC32C) before the chunks are reported.  The chunk in which the first invalid batch begins, and every chunk behind it, have
     * status {@link #E_RECORDS}.  Detransform accepts and ignores the flag.
     */
    public static final int VALIDATE_RECORDS = 0x100;
    /**
     * With {@link #VALIDATE_RECORDS} on {@code transformBatch} ({@code segment.records.validate.frames}): every batch that has passed its
     * CRC is examined further - the order of base offsets from batch to batch, the record count, and for an uncompressed batch the varint
     * framing and the offset deltas of every record.  Without {@link #VALIDATE_RECORDS} the call is refused; the streamed form
     * ({@code transformBatchStream}) refuses the flag.  Detransform accepts and ignores it.
     */
    public static final int VALIDATE_FRAMES = 0x400;

    public static final int OK = 0;
    public static final int E_TAG_MISMATCH = -5;
    public static final int E_BAD_FRAME = -6;
    public static final int E_BAD_SIZE = -7;
    /** Under {@link #VERIFY} / {@link #VERIFY_GCM}: what was written for this chunk does not restore it (per chunk; the batch call itself succeeds). */
    public static final int E_VERIFY = -10;
    /** Under {@link #VALIDATE_RECORDS}: an invalid record batch begins in or before this chunk of the source (per chunk; the batch call itself succeeds). */
    public static final int E_RECORDS = -11;

    /** Size of one tsx_chunk_desc (include/tsxform.h), written/read through a direct little-endian ByteBuffer. */
    public static final int DESC_BYTES = 48;
    public static final int DESC_SRC_OFF = 0;
    public static final int DESC_DST_OFF = 8;
    public static final int DESC_SRC_LEN = 16;
    public static final int DESC_DST_CAP = 20;
    public static final int DESC_DST_LEN = 24;
    public static final int DESC_CRC32C = 28;
    public static final int DESC_STATUS = 32;
    public static final int DESC_IV = 36;

    /**
     * TSX_ZSTD_PROFILE_*: which libzstd behaviour the compressor reproduces (INTEGRATION.md, "Zstd profile").  1_5_7 is byte-identical to
     * the real 1.5.7; 1_5_6 is 1.5.7 without its pre-block splitter - an unverified stand-in for the 1.5.6 inside zstd-jni 1.5.6-9.
     */
    public static final int ZSTD_PROFILE_1_5_6 = 0;
    public static final int ZSTD_PROFILE_1_5_7 = 1;
    /**
     * TSX_ZSTD_PROFILE_DEVICE: standard Zstandard frames from a parse shaped for the GPU (64 lanes parse 64 slices of a block side by
     * side) - no libzstd's bytes, larger than level 3's frames, readable by every Zstandard decoder, the same bytes for the same chunk
     * on every run.  It has no levels: {@code compression.zstd.level} together with it is refused.  {@code compression.zstd.verify=true}
     * is recommended with it: its frames have no library to be compared with, and verify on upload decodes every one of them against
     * its chunk before the segment is reported.
     */
    public static final int ZSTD_PROFILE_DEVICE = 2;

    /** The value of the configuration key {@code gpu.zstd.profile}: {@code 1.5.6}, {@code 1.5.7} or {@code device}. */
    public static int zstdProfileOf(final String configured) {
        switch (configured) {
            case "1.5.6": return ZSTD_PROFILE_1_5_6;
            case "1.5.7": return ZSTD_PROFILE_1_5_7;
            case "device": return ZSTD_PROFILE_DEVICE;
            default: throw new IllegalArgumentException("gpu.zstd.profile must be 1.5.6, 1.5.7 or device, " + configured + " given");
        }
    }

    static {
        System.loadLibrary("tsxform_jni");   // links libtsxform.so
        final int devices = init();
        if (devices <= 0) {
            // there is no CPU implementation behind this binding
            throw new UnsatisfiedLinkError("tsxform: no usable gfx950 device: " + strerror(devices));
        }
    }

    private TsxNative() {
    }

    /** tsx_init(0, NULL): all visible devices. */
    private static native int init();

    public static native String strerror(int code);

    /** tsx_device_count: GPUs the library drives (all visible ones). */
    public static native int deviceCount();

    /** tsx_set_thread_device: device of the calling thread's batches, -1 = the least loaded one. */
    public static native int setThreadDevice(int device);

    /** tsx_host_register / tsx_host_unregister: pin a direct buffer that is reused for batches. */
    public static native int hostRegister(ByteBuffer buf);

    public static native int hostUnregister(ByteBuffer buf);

    /**
     * Per-thread, grow-only direct buffers (src, dst, descriptors) of the calling thread, pinned once per (re)allocation:
     * no off-heap allocation and no page faults on the hot path, and the copies go by DMA.
     */
    public static final class Buffers {
        private static final ThreadLocal<Buffers> LOCAL = ThreadLocal.withInitial(Buffers::new);
        private ByteBuffer src;
        private ByteBuffer dst;
        private ByteBuffer descs;

        public static Buffers get() {
            return LOCAL.get();
        }

        private static ByteBuffer grow(final ByteBuffer old, final long need, final boolean pin) {
            if (need > Integer.MAX_VALUE - 64) {
                // one direct ByteBuffer holds < 2 GiB: the batch size is bounded at construction time of the enumerations
                throw new IllegalArgumentException("batch of " + need + " bytes exceeds a direct ByteBuffer");
            }
            if (old != null && old.capacity() >= need) {
                old.clear();
                return old;
            }
            if (old != null && pin) {
                hostUnregister(old);
            }
            final ByteBuffer fresh = ByteBuffer.allocateDirect((int) Math.min(need + need / 8 + 64, (long) Integer.MAX_VALUE - 64))
                .order(java.nio.ByteOrder.LITTLE_ENDIAN);          // headroom for the next, slightly larger batch - never beyond what one buffer holds
            if (pin) {
                hostRegister(fresh);          // best effort: an unpinned buffer still works (runtime-staged copies)
            }
            return fresh;
        }

        public ByteBuffer src(final long need) {
            src = grow(src, need, true);
            return src;
        }

        public ByteBuffer dst(final long need) {
            dst = grow(dst, need, true);
            return dst;
        }

        public ByteBuffer descs(final int n) {
            descs = grow(descs, (long) n * DESC_BYTES, false);
            return descs;
        }

        /**
         * For a thread that is about to end (the broker's upload / fetch threads and the read-ahead helpers never do): the
         * pinning must be undone before the garbage collector frees the buffers' memory.
         */
        public static void release() {
            final Buffers b = LOCAL.get();
            if (b.src != null) {
                hostUnregister(b.src);
            }
            if (b.dst != null) {
                hostUnregister(b.dst);
            }
            b.src = null;
            b.dst = null;
            b.descs = null;
            LOCAL.remove();
        }
    }

    /** tsx_transformed_bound. */
    public static native long transformedBound(long n, int flags);

    /**
     * tsx_transform_batch / tsx_detransform_batch over direct buffers (host memory, TSX_MEM_HOST) with a pooled context.
     *
     * @param descs n * DESC_BYTES, little-endian, in/out
     * @param key   32-byte AES key or null; zeroised in native memory before returning
     * @return batch-level status (0 or a negative TSX_E_* code); per-chunk status is in descs
     */
    public static native int transformBatch(int flags, byte[] key, byte[] aad, int zstdProfile,
                                            ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst);

    /**
     * tsx_transform_batch with TSX_MEM_HOST_PACKED: the transformed chunks are written back to back into {@code dst} - the
     * upload's own buffer (a multipart part, TransformFinisher's object) - and each descriptor returns its chunk's offset and
     * size; a chunk that does not fit any more comes back with TSX_E_DST_TOO_SMALL.
     */
    public static native int transformBatchPacked(int flags, byte[] key, byte[] aad, int zstdProfile,
                                                  ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst);

    /**
     * {@link #transformBatch} and {@link #transformBatchPacked} at a Zstandard level ({@code compression.zstd.level}): 1, 2 or 3, or 0
     * for the library default (3, what the reference's zstd-jni call uses).  Any other level returns TSX_E_UNSUPPORTED, as does a
     * library older than these methods for 1 and 2.
     */
    public static native int transformBatchLevel(int flags, byte[] key, byte[] aad, int zstdProfile, int zstdLevel,
                                                 ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst);

    public static native int transformBatchPackedLevel(int flags, byte[] key, byte[] aad, int zstdProfile, int zstdLevel,
                                                       ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst);

    public static native int detransformBatch(int flags, byte[] key, byte[] aad,
                                              ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst);

    /** Size of a tsx_records_state (include/tsxform.h): the state of one segment that is validated over several batches. */
    public static final int RECORDS_STATE_BYTES = 192;
    /** Size of a tsx_records_info and where its fields lie (little-endian). */
    public static final int RECORDS_INFO_BYTES = 40;
    public static final int RECORDS_INFO_BATCHES = 0;
    public static final int RECORDS_INFO_COMPRESSED_BATCHES = 8;
    public static final int RECORDS_INFO_FIRST_BAD_POS = 16;
    public static final int RECORDS_INFO_FIRST_BAD_REASON = 24;

    /** tsx_records_begin: {@code state} describes a stream of {@code streamBytes} bytes in all (the segment's size) of which none has been seen. */
    public static native int recordsBegin(ByteBuffer state, long streamBytes);

    /**
     * tsx_transform_batch_stream, slot layout and packed: {@link #transformBatchLevel} / {@link #transformBatchPackedLevel} whose chunks
     * CONTINUE the stream {@code state} describes ({@code flags} must contain {@link #VALIDATE_RECORDS}).  The state is the caller's:
     * consecutive batches may run on any thread, one after another.  A negative return leaves it as it was.
     */
    public static native int transformBatchStream(int flags, byte[] key, byte[] aad, int zstdProfile, int zstdLevel,
                                                  ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst, ByteBuffer state);

    public static native int transformBatchPackedStream(int flags, byte[] key, byte[] aad, int zstdProfile, int zstdLevel,
                                                        ByteBuffer descs, int n, ByteBuffer src, ByteBuffer dst, ByteBuffer state);

    /**
     * tsx_records_result: 1 when the stream is complete (the bytes consumed equal the declared length), 0 when it is not, negative for a
     * state that was never begun; {@code info} (a direct little-endian buffer of {@link #RECORDS_INFO_BYTES}) receives the tsx_records_info
     * of the stream so far.
     */
    public static native int recordsResult(ByteBuffer state, ByteBuffer info);
}
