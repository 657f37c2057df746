/*
 * tsxform — C ABI of the MI355X-native chunk-transform library (libtsxform.so).
 *
 * This is the drop-in boundary for the hot path of aiven/tiered-storage-for-apache-kafka:
 * the per-chunk  compress -> AES-256-GCM encrypt (-> CRC32C)  chain of copyLogSegmentData() and its
 * inverse in fetchLogSegment().  A JNI shim (java/ sources) binds exactly these entry
 * points from GpuTransformChunkEnumeration / GpuDetransformChunkEnumeration / GpuChunkManager, which
 * implement the reference's own interfaces:
 *   core/src/main/java/io/aiven/kafka/tieredstorage/transform/TransformChunkEnumeration.java:28-42
 *   core/src/main/java/io/aiven/kafka/tieredstorage/transform/DetransformChunkEnumeration.java:28
 *   core/src/main/java/io/aiven/kafka/tieredstorage/fetch/ChunkManager.java:26-31
 *
 * Conventions: plain pointers and sizes only; caller owns every buffer; the library never keeps a
 * caller pointer after a call returns; nothing throws across the ABI.  Batch-level failures are the
 * (negative) return value; per-chunk failures are tsx_chunk_desc.status.  All entry points are
 * re-entrant: a tsx_ctx is a per-thread handle (own HIP stream + device workspace), and the
 * ctx-less convenience calls take one from an internal pool (reference threading: >=10 RLM upload
 * threads + the ChunkCache ForkJoinPool call concurrently).
 *
 * There is NO CPU implementation behind this ABI: without a usable gfx950 device tsx_init() fails
 * with TSX_E_DEVICE and every compute entry point returns TSX_E_DEVICE.
 */
#ifndef TSXFORM_H
#define TSXFORM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSX_ABI_VERSION 4 /* 2: ctx-less calls spread over all initialised devices; tsx_set_thread_device, tsx_host_register
                             3: the batch entry points take src_size and reject descriptors that reach beyond it
                             4: tsx_init_ex / tsx_config, tsx_service_stats, tsx_service_quiesce (the compressor service) */

/* flags: which stages of the chain run.  Replaces the reference's chain construction
 * RemoteStorageManager.transformation(), core/.../RemoteStorageManager.java:434-453
 * (Base -> [Compression] -> [Encryption]) and DefaultChunkManager.getChunk(),
 * core/.../fetch/DefaultChunkManager.java:56-67 (Base -> [Decryption] -> [Decompression]). */
#define TSX_COMPRESS 0x1u /* Zstd frame per chunk   (CompressionChunkEnumeration.java:50-63)      */
#define TSX_ENCRYPT  0x2u /* IV||C||TAG, AES-256-GCM (EncryptionChunkEnumeration.java:66-84)       */
#define TSX_CRC      0x4u /* CRC32C of the ORIGINAL chunk bytes, out of band       */
/* Modifier of TSX_COMPRESS on transform: every frame carries a content checksum (ZSTD_c_checksumFlag: descriptor bit 2, and
 * behind the last block the low 32 bits of XXH64 of the chunk), byte for byte libzstd's frame with that flag.  Without
 * TSX_COMPRESS it is TSX_E_INVAL.  Detransform accepts and ignores it: there the FRAME decides - a frame that declares a checksum
 * is always verified, and a mismatch is TSX_E_BAD_FRAME (zstd-jni: "Restored data doesn't match checksum").
 * tsx_transformed_bound covers the four bytes. */
#define TSX_ZSTD_CHECKSUM 0x8u
/* Modifier of TSX_COMPRESS on transform: verify on upload.  Every Zstandard frame the device has written is read back by the decoder's
 * own parsing code and compared with the chunk it was written from, before the chunk is reported: a chunk whose frame does not restore
 * it byte for byte (or whose content checksum is not the chunk's) gets status TSX_E_VERIFY and dst_len 0; the call still returns TSX_OK
 * and the other chunks are delivered.  With the flag set no chunk is reported TSX_OK unverified (TSX_E_NOMEM when the verifier finds no
 * memory).  Scope: the Zstandard frame.  The AES-GCM stage behind it is NOT covered by this flag, nor is the copy of the frame into the
 * caller's buffer: TSX_VERIFY_GCM below examines the bytes handed back.  While verifying uploads run, the compute units reserved for fetches
 * stay reserved (the verifier's kernels are ordinary kernels: tsx_config.fetch_quiet_ms).  On a verifying transform tsx_timing's
 * unzstd_ms / unzstd_launches are the verifier's.  Without TSX_COMPRESS it is TSX_E_INVAL; detransform accepts and ignores it
 * (callers build one flags word for both directions).  (0x10 stays unassigned.) */
#define TSX_VERIFY 0x20u
/* Modifier of TSX_ENCRYPT on transform: verify on upload, AES-GCM stage.  Every chunk that is TSX_OK behind the GCM stage is examined
 * on the device, in the bytes the device DELIVERED - IV || C || TAG where it wrote them: the caller's device buffer, the context's
 * output buffer (copy path), or the caller's registered host buffer (zero-copy output, read back over PCIe) - before it is reported:
 *   dst_len is the plaintext length + 28; the 12 delivered IV bytes are descs[i].iv; AES-256-CTR of the delivered ciphertext under the
 *   batch key and that IV is, byte for byte, the plaintext the stage was given (the chunk's Zstandard frame in the staging buffer when
 *   compressing, the chunk's source bytes on the device otherwise); GHASH over the AAD, the delivered ciphertext and the length block,
 *   xor E_K(J0), is the delivered tag.
 * A chunk that fails gets status TSX_E_VERIFY and dst_len 0; the call still returns TSX_OK and the other chunks are delivered (TSX_VERIFY's
 * semantics).  With the flag set no chunk is reported TSX_OK unexamined (TSX_E_NOMEM when the verifier finds no memory for its verdicts).
 * With TSX_VERIFY as well the Zstandard verifier runs first and the chunks it failed are skipped; the chain is then
 * source == decode(frame), frame == decrypt(delivered), tag valid.  Valid with or without TSX_COMPRESS (encrypt-only uploads), TSX_CRC,
 * TSX_ZSTD_CHECKSUM and TSX_VERIFY; without TSX_ENCRYPT it is TSX_E_INVAL; detransform accepts and ignores it.  The verifier's kernels are
 * ordinary kernels (next to the compressor service the batch counts as a fetch having been seen: the reserved compute units stay
 * reserved) and add to tsx_timing's gcm_ms / gcm_launches.
 * NOT covered: the copy engine's device-to-host copy on the copy path (a destination the device cannot address); the host's memmove of a
 * packed batch that is packed down in place; a common-mode error of the AES and GHASH device functions, which the encrypting and the
 * verifying kernels share (the test suite's comparison with OpenSSL guards those).  (0x10 and 0x40 stay unassigned.) */
#define TSX_VERIFY_GCM 0x80u
/* Modifier of a transform with any stage combination: validate the SOURCE as a Kafka log before it is uploaded.  The batch's chunks,
 * concatenated in descriptor order ([src_off, src_off + src_len) of chunk 0, 1, ...; gaps between slots are not part of it, chunks of
 * length 0 contribute nothing), are taken as ONE byte stream that begins on a record-batch boundary and ends on one - a whole segment in
 * one call; a segment split over several calls goes through tsx_transform_batch_stream below.  Every batch of the stream is checked on the device the way
 * DefaultRecordBatch.ensureValid() plus a walk over the log would check it (fields big-endian: baseOffset @0, batchLength @8,
 * partitionLeaderEpoch @12, magic @16, crc @17, attributes @21 ...):
 *   at least 61 bytes are left in the stream; batchLength >= 49 as a signed 32-bit value; position + 12 + batchLength <= the stream's
 *   length; magic == 2; CRC32C (java.util.zip.CRC32C) over [position + 21, position + 12 + batchLength) equals the crc field; the stream
 *   ends exactly at the end of a batch.  (Bytes 0..15 are outside the CRC: damage there, other than to the length, does not fail.)
 * The first invalid batch decides: the chunk that holds its first byte, and every chunk after it, get status TSX_E_RECORDS and dst_len 0
 * (a chunk that already carries another error keeps it); earlier chunks are delivered; the call returns TSX_OK, as with TSX_VERIFY.  With
 * the flag set no chunk is reported TSX_OK whose bytes the validator has not covered (TSX_E_NOMEM when it finds no memory).  The
 * validator's kernels are ordinary kernels that run while the batch's own stages do (next to the compressor service the batch counts as
 * a fetch having been seen); tsx_ctx_records() describes what they found.  With the flag clear nothing is allocated or launched.
 * Covered only with TSX_VALIDATE_FRAMES (below): the framing of the records inside a batch and the order of offsets.  NOT covered with
 * either flag: compressed payloads; message sets of magic 0 / 1 fail (reason 3).  Detransform accepts and ignores the flag.  (0x10 and
 * 0x40 stay unassigned.) */
#define TSX_VALIDATE_RECORDS 0x100u
/* Modifier of TSX_VALIDATE_RECORDS on tsx_transform_batch (without it: TSX_E_INVAL): every batch that has passed its CRC is examined
 * further, in stream order, and counts as valid only if it passes.  The first failing check of the first failing batch decides, with
 * the same statuses as above.  Header fields big-endian: baseOffset i64 @0, lastOffsetDelta i32 @23, recordsCount i32 @57; the records
 * occupy [position + 61, the batch's end).
 *   1. offsets (reason 6): baseOffset >= 0; lastOffsetDelta >= 0; baseOffset + lastOffsetDelta does not overflow an i64; baseOffset is
 *      greater than the baseOffset + lastOffsetDelta of the valid batch in front (the stream's first batch has none).  Every batch,
 *      compressed ones included.  This is what catches damage to baseOffset, which lies outside the CRC - as far as it breaks the order:
 *      a flipped low bit that leaves the batch between its neighbours passes.
 *   2. count (reason 5): recordsCount >= 0.
 *   3. records, of an uncompressed batch (attributes & 7 == 0; control batches included): exactly recordsCount records are read from
 *      position + 61 the way DefaultRecord.readFrom reads them - varints and varlongs as ByteUtils.readVarint / readVarlong (zigzag; at
 *      most 5 / 10 bytes, a continuation bit on the last is malformed; excess bits of a 5th byte are dropped).  Per record, in wire order:
 *      length >= 0 and the body inside the batch; attributes; timestampDelta; offsetDelta with 0 <= delta <= lastOffsetDelta and greater
 *      than the record's in front (a violation is reason 6); keyLength >= -1 and the key; valueLength >= -1 and the value; headersCount
 *      >= 0, per header a key length >= 0 with its bytes and a value length >= -1 with its bytes; the fields end exactly at the body's end.
 *      A field that would leave its record, or a record its batch, is a verdict, never an address.  Everything but the offsetDelta rule
 *      is reason 5.  The lowest-numbered failing record decides, within it the first failing field.  Behind the last record the position
 *      must be the batch's end (reason 5).  An empty batch (recordsCount 0, nothing behind the header), as compaction leaves them, passes
 *      whatever its lastOffsetDelta.
 * NOT checked: timestamps, the order of partitionLeaderEpoch, producer id / epoch / sequence, the payloads of compressed batches - and
 * the streamed form: tsx_transform_batch_stream refuses the flag with TSX_E_UNSUPPORTED (the records of a batch that is open across two
 * calls cannot be walked without buffering the batch).  A record is read by one lane: a hostile batch that is ONE record of a GiB of
 * empty headers, sealed with a valid CRC, costs that lane a walk over all of it.  Detransform accepts and ignores the flag.  With the
 * flag clear nothing changes - the same kernels, launches and allocations.  (0x10, 0x40 and 0x200 stay unassigned.) */
#define TSX_VALIDATE_FRAMES 0x400u

/* where src/dst live */
/* host pointers.  The batch is cut into pieces whose H2D copy, kernels and D2H copy overlap: pieces of >= 64 MiB in order on three
 * streams of the ctx; a compressing batch goes as up to 4 members of the device's compressor service (a chunk is ~1 s of one wave whatever
 * the batch size: piece k is published when its share of the input has landed, its output travels while later pieces run).  Any host memory
 * works - pageable buffers are staged by the HIP runtime; buffers pinned once with tsx_host_register() are copied by DMA without a staging pass.
 * A compressing batch whose WHOLE dst buffer the device can address (inside one tsx_host_register'ed buffer, or one hipHostMalloc'ed
 * allocation) has no output copy at all: the device writes every chunk's transformed bytes straight into [dst_off, dst_off + dst_len)
 * during the call (nothing beyond dst_len is written; what the buffer holds is defined when the call returns, as for any other kind).
 * A dst of which only a part is registered takes the copy path. */
#define TSX_MEM_HOST   0
/* device pointers (same HIP runtime / process): no copies.  The kernels run on the ctx's own streams: work the caller still has
 * queued on other streams for these buffers (the kernel that fills src, a memset of dst) must be complete when the call is made,
 * and the call returns when the library's work is complete. */
#define TSX_MEM_DEVICE 1
/* host pointers, transformed chunks written BACK TO BACK into dst in batch order - the bytes of the `.log` object (or of a
 * multipart part buffer) exactly as TransformFinisher.java:134-151 (SequenceInputStream over the chunks) hands them to
 * ObjectUploader.upload / S3MultiPartOutputStream.java:89-122, without the bound-sized slot per chunk and the gather copy
 * behind it.  tsx_transform_batch only.  descs[i].dst_off / dst_cap are ignored on entry; on return dst_off is chunk i's
 * offset in dst and dst_len its size; a chunk that no longer fits dst_size gets TSX_E_DST_TOO_SMALL (and so do all after it).
 * The bytes of dst BEHIND the packed chunks are scratch: when dst_size has room for one bound-sized slot per chunk and the device can
 * address dst, the chunks are written there first and packed down in place (no device output buffer, no copies). */
#define TSX_MEM_HOST_PACKED 2

/* status / error codes (0 = ok, negative = error) */
#define TSX_OK               0
#define TSX_E_INVAL         -1  /* bad argument                                                   */
#define TSX_E_DEVICE        -2  /* no usable gfx950 device / HIP failure                          */
#define TSX_E_NOMEM         -3
#define TSX_E_DST_TOO_SMALL -4  /* dst_cap < transformed size                                     */
#define TSX_E_TAG_MISMATCH  -5  /* GCM tag check failed  (JCE AEADBadTagException,
                                   DecryptionChunkEnumeration.java:59-61)                           */
#define TSX_E_BAD_FRAME     -6  /* corrupt Zstd frame (zstd-jni ZstdException)                    */
#define TSX_E_BAD_SIZE      -7  /* frame without usable content size: reference throws
                                   "Invalid decompressed size: n" (DecompressionChunkEnumeration.java:42-44) */
#define TSX_E_SHORT_CHUNK   -8  /* encrypted chunk shorter than IV+TAG                            */
#define TSX_E_UNSUPPORTED   -9
#define TSX_E_VERIFY        -10 /* TSX_VERIFY / TSX_VERIFY_GCM: the frame written for this chunk does not restore it (per chunk)  */
#define TSX_E_RECORDS       -11 /* TSX_VALIDATE_RECORDS: the source holds an invalid record batch in or before this chunk (per chunk) */

/* Per-chunk descriptor; mirrors io.aiven.kafka.tieredstorage.Chunk (core/.../Chunk.java:21-36:
 * id, originalPosition, originalSize, transformedPosition, transformedSize) with the in/out split
 * a batch call needs.  48 bytes, no padding. */
typedef struct tsx_chunk_desc {
    uint64_t src_off;  /* in : offset of this chunk's input within src                              */
    uint64_t dst_off;  /* in : offset of this chunk's output slot within dst                        */
    uint32_t src_len;  /* in : input bytes (originalSize on transform, transformedSize on detransform) */
    uint32_t dst_cap;  /* in : capacity of the output slot                                          */
    uint32_t dst_len;  /* out: bytes produced; 0 when status != TSX_OK - what the chunk's slot (or, packed, the buffer behind
                               the packed chunks) then holds is undefined: with zero-copy output a failed chunk's bytes
                               may already have been written there                                          */
    uint32_t crc32c;   /* out: CRC32C of the original (pre-transform / restored) bytes if TSX_CRC   */
    int32_t  status;   /* out: TSX_OK or a TSX_E_* code for this chunk                              */
    uint8_t  iv[12];   /* in : GCM IV for transform (host SecureRandom, AesEncryptionProvider.java:66-71);
                          detransform reads the IV from the chunk's first 12 bytes and ignores this    */
} tsx_chunk_desc;

/* Per-batch parameters: one (data key, AAD) pair per segment
 * (AesEncryptionProvider.createDataKeyAndAAD, core/.../security/AesEncryptionProvider.java:52-58). */
typedef struct tsx_batch_params {
    uint32_t flags;        /* TSX_COMPRESS | TSX_ENCRYPT | TSX_CRC [| TSX_ZSTD_CHECKSUM] [| TSX_VERIFY] [| TSX_VERIFY_GCM] [| TSX_VALIDATE_RECORDS [| TSX_VALIDATE_FRAMES]] */
    uint32_t aad_len;      /* reference: 32                                                         */
    uint8_t  key[32];      /* AES-256 data key (SecretKey.getEncoded())                             */
    uint8_t  aad[64];
    int32_t  zstd_level;   /* 0 = library default (3), what the reference uses; 1, 2, 3 are implemented (frames byte for byte
                            * libzstd's at that level); anything else is TSX_E_UNSUPPORTED.  Members of different levels share the
                            * device's compressor service; tsx_transformed_bound does not depend on the level                    */
    uint32_t zstd_profile; /* TSX_ZSTD_PROFILE_*                                                    */
} tsx_batch_params;

/* Which libzstd behaviour the compressor reproduces.  TSX_ZSTD_PROFILE_1_5_7: byte for byte the real libzstd 1.5.7 (checked against
 * the library itself on every test input).  TSX_ZSTD_PROFILE_1_5_6: the same code WITHOUT 1.5.7's pre-block splitter - an UNVERIFIED
 * stand-in for the release the reference ships (1.5.6 inside zstd-jni 1.5.6-9, core/build.gradle:29): no libzstd 1.5.6 exists in the
 * build or test environment, and the 1.5.7 release notes may list more level-3 changes than the splitter (a ratio improvement of the
 * double-fast parser has been recalled by a reviewer; neither recollection could be checked).  Frames are valid Zstandard either way;
 * whether they are 1.5.6's bytes is settled where that library exists: tests/golden/make_vectors_from_lib.py + tests/test_golden.py. */
#define TSX_ZSTD_PROFILE_1_5_6 0u
#define TSX_ZSTD_PROFILE_1_5_7 1u
/* TSX_ZSTD_PROFILE_DEVICE: standard Zstandard frames (RFC 8878) that are NOT any libzstd's bytes.  The frame header, the 128 KiB blocks
 * (cut at fixed 128 KiB, no pre-splitter), the window (at most 1 << 21), the raw and RLE fallbacks, the entropy stages, the content
 * checksum on TSX_ZSTD_CHECKSUM and tsx_transformed_bound are those of the other profiles; the match finder is a parse shaped for the
 * wave: 64 lanes parse 64 slices of a block side by side, with 64 table probes in flight where the exact parse has one dependency chain.
 * Every Zstandard decoder reads the frames, and a frame is a function of the chunk's bytes and the flags only - the same on every run,
 * wave and device.  What it is not: byte-identical to any library, as small as level 3's frames (DESIGN.md has the ratios), or
 * selectable by level - zstd_level must be 0 with it, anything else is TSX_E_UNSUPPORTED (levels name libzstd's parsers).
 * tsx_detransform_batch ignores the profile.  TSX_VERIFY is recommended with it: the frames have no library to be compared against. */
#define TSX_ZSTD_PROFILE_DEVICE 2u

typedef struct tsx_ctx tsx_ctx;

/* Timing of the last batch on a ctx, measured with HIP events on the ctx's own stream. */
typedef struct tsx_timing {
    float total_ms;    /* first enqueue -> last kernel/copy done                                    */
    float h2d_ms, d2h_ms;
    float crc_ms, zstd_ms, gcm_ms, unzstd_ms;
    uint32_t crc_launches, zstd_launches, gcm_launches, unzstd_launches;
} tsx_timing;

/* ---- library lifetime ---------------------------------------------------------------------- */
uint32_t    tsx_abi_version(void);
const char* tsx_version(void);           /* "tsxform x.y (gfx950; zstd parity target 1.5.7/1.5.6, levels 1-3, device profile)" */
const char* tsx_strerror(int code);
/* device_ids == NULL: use devices 0..device_count-1; device_count <= 0: all visible devices.  An id may be listed more than once
 * (the same GPU as several logical devices, each with its own pools and compressor service: tests of the multi-device dispatch).
 * Returns the number of devices in use (>0) or TSX_E_DEVICE. */
int  tsx_init(int device_count, const int* device_ids);

/* What a deployment may want to say about the device-side machinery; TSX_CFG_DEFAULT(64) in a field = the library's default.
 * The environment of the process, read once inside tsx_init(_ex), overrides both: TSX_FETCH_RESERVED_CUS,
 * TSX_FETCH_SHARED_CU_WAVES, TSX_FETCH_QUIET_MS, TSX_SERVICE_MAX_LAUNCH_MS, TSX_POOL_IDLE_BYTES.  Nothing on a data path reads the environment. */
#define TSX_CFG_DEFAULT   0xFFFFFFFFu
#define TSX_CFG_DEFAULT64 0xFFFFFFFFFFFFFFFFull
typedef struct tsx_config {
    uint32_t struct_size;            /* sizeof(tsx_config) as the caller was compiled                                           */
    uint32_t fetch_reserved_cus;     /* compute units the compressor never occupies, so that a fetch (fetchLogSegment ->
                                        ChunkCache.java:85-108, get.timeout.ms 10 s) finds room at once while uploads fill the
                                        chip.  Default: one per SHADER ENGINE (32 of an MI355X's 256) - the hardware hands a
                                        kernel's workgroups to the engines in turn and a workgroup waits for room in its own;
                                        a smaller number is spread over the engines and leaves some without a free CU (a fetch
                                        can then wait for the end of a compressor launch); 0 = no reservation                  */
    uint32_t service_max_launch_ms;  /* one launch of the compressor service kernel stops taking chunks at this age (the next
                                        launch takes over): bounds how long a device-wide synchronisation made by OTHER code in
                                        the process (hipFree, hipDeviceSynchronize) can wait under continuous uploads; default
                                        60000, 0 = no limit                                                                   */
    uint32_t fetch_shared_cu_waves;  /* compressor waves that stay on each reserved CU all the same (0 / default: none - the CU is left
                                        alone).  A trade, measured under 5 upload callers (profiles/r05_keep_waves_on_reserved_cus.jsonl):
                                        4 -> uploads + 3 %, a 4 MiB fetch 2.8 -> 3.7 ms; 8 -> + 6 %, 4.2 ms, and now and then a fetch that
                                        waits ~0.5 s for the compressor launch to be rotated; 12 and more: such waits become regular.
                                        At most 8 is accepted                                                                  */
    uint64_t pool_idle_bytes;        /* idle pooled workspace kept per device; default 4/9 of its memory                      */
    uint32_t fetch_quiet_ms;         /* the reservation follows the traffic (default 2000; 0 = the reserved CUs are never used by the
                                        compressor).  Once no fetch (no batch of ordinary kernels) has run for this long, a launch of the
                                        compressor's kernel has waves on the reserved CUs too, as GUESTS: they work for as long as the
                                        queue has work for them - a chip that is full AND busy is what they are for; a guest that finds
                                        the queue dry for 10 ms (500 while most of the chip is busy) gives its slot back - and the next fetch makes them hand their chunks
                                        back and leave, which costs that ONE fetch a block time of a chunk (~30 ms); the CUs then stay
                                        reserved until it has been quiet again.  Measured (round 6, MI355X): bench.py value 18.2 -> 20.5,
                                        continuously fed 19.8 -> 22.3 GiB/s.  Why it was opt-in in round 5 and what was wrong then:
                                        profiles/r06_guest_waves_root_cause.md, r06_full_chip_with_idle_waves.txt                      */
    uint32_t reserved2_;
} tsx_config;
int  tsx_init_ex(int device_count, const int* device_ids, const tsx_config* cfg);   /* cfg == NULL: tsx_init */
/* Every tsx_ctx must have been destroyed and no batch may be in flight.  No entry point of this library changes the calling
 * thread's current HIP device: each one that selects a device puts the previous one back before it returns. */
void tsx_shutdown(void);
int  tsx_device_count(void);

/* ---- contexts ------------------------------------------------------------------------------ */
/* max_chunks/max_chunk_size size the device workspace (grown on demand when exceeded). */
int  tsx_ctx_create(int device_index, uint32_t max_chunks, uint32_t max_chunk_size, tsx_ctx** out);
void tsx_ctx_destroy(tsx_ctx* ctx);
int  tsx_ctx_timing(const tsx_ctx* ctx, tsx_timing* out);
/* What TSX_VALIDATE_RECORDS found in the last batch on a ctx (explicit contexts only; all zero, first_bad_pos UINT64_MAX, when that
 * batch did not validate). */
typedef struct tsx_records_info {
    uint64_t batches;             /* valid batches in front of the first invalid one (all of them in a clean stream)                 */
    uint64_t compressed_batches;  /* ... of which attributes & 7 != 0 (what compression.heuristic.enabled asks, for the whole segment) */
    uint64_t first_bad_pos;       /* stream offset of the first invalid batch, or UINT64_MAX                                         */
    uint32_t first_bad_reason;    /* 0 none; 1 truncated (fewer than 61 bytes left, or the batch reaches beyond the stream's end);
                                     2 length (batchLength < 49); 3 magic; 4 crc; with TSX_VALIDATE_FRAMES also 5 records (the
                                     count or the framing of the batch's records) and 6 offsets (of the batch or of a record)        */
    uint32_t repaired_chunks;     /* chunks whose batches the resolver walked itself: the chunk's own walker had found no entry, or
                                     another one than the chain arrives at (a CRC-valid batch inside a record value, a damaged first
                                     batch)                                                                                          */
    float    ms;                  /* the validator's kernels, by events                                                              */
    uint32_t records;             /* TSX_VALIDATE_FRAMES: sum of recordsCount over the valid uncompressed batches in front of the first
                                     invalid batch - the records actually read (saturates at UINT32_MAX); 0 without the flag         */
} tsx_records_info;
int  tsx_ctx_records(const tsx_ctx* ctx, tsx_records_info* out);
int  tsx_ctx_device(const tsx_ctx* ctx);                /* device index (0 .. tsx_device_count()-1) the ctx lives on */

/* Device of the calling thread's ctx-less calls: 0 .. tsx_device_count()-1, or -1 = automatic (least loaded).  The JVM side
 * passes  segment hash % devices  so that the chunks of one segment stay on one GPU (segment s -> GPU s mod N). */
int  tsx_set_thread_device(int device_index);
/* Pool of the ctx-less calls on one device: idle contexts kept (at most 32, and at most 128 GiB of device workspace between them),
 * contexts out right now, batches served so far. */
int  tsx_pool_stats(int device_index, uint32_t* idle, uint32_t* in_use, uint64_t* batches);

/* The compressor service of a device (every compressing batch is a member of ONE device-wide queue that persistent waves pull
 * chunks from; csrc/tsx_internal.h).  Counters since tsx_init; kernel_ms is the device's own clock (the last wave of a launch reports its begin and end through pinned memory). */
typedef struct tsx_service_info {
    uint64_t launches;           /* launches of the service kernel that have been started                                       */
    uint64_t watchdog_launches;  /* ... of which a waiting caller made because the kernel had ended with work still queued       */
    uint64_t members, chunks;    /* batches (pieces) published / chunks of completed members                                     */
    double   kernel_ms;          /* summed duration of the launches that have ENDED                                              */
    uint32_t running;            /* 1: a launch is out right now                                                                 */
    uint32_t waves;              /* one-wave workgroups per launch                                                               */
    uint32_t compute_units, cu_keys_seen, reserved_cus;   /* CUs of the device, distinct CU ids a probe launch met, CUs left alone */
    uint32_t device_chunks, wave_starts, reserved_exits, skipped_tickets;   /* device-side counters (mod 2^32)                   */
    uint32_t live_waves, live_waves_max;   /* waves of the service resident right now / the most ever                              */
    uint32_t shader_engines;               /* shader engines the probe launch met (groups of CUs the hardware fills separately)        */
    uint32_t rotations;                    /* launches a fetch that had waited 200 ms asked to end early (the safety net of the fetch side) */
    uint32_t guest_launches;               /* launches whose waves used the reserved CUs too (no fetch had been seen for fetch_quiet_ms)  */
    uint32_t yielded_waves;                /* guest waves that handed their chunk back and left when a fetch arrived                      */
    uint32_t returned_chunks;              /* ... chunks handed back that way (each was started again by another wave)                   */
    uint32_t readmissions;                 /* launches asked to end so that the next one could use the reserved CUs again (quiet again)   */
    uint32_t relocated_waves;              /* compressor waves that found themselves on a reserved CU they had not started on (the hardware's
                                              scheduler saves and restores waves), handed their chunk back and left.  (Occupies what was the
                                              struct's tail padding: its size, 112 bytes, is what it was.)                                  */
} tsx_service_info;
int  tsx_service_stats(int device_index, tsx_service_info* out);
/* Returns when the device's service kernel has ended (a moment after its last chunk): brackets a measurement. */
int  tsx_service_quiesce(int device_index);

/* Pin / unpin a host buffer that is reused for TSX_MEM_HOST(_PACKED) batches (hipHostRegister): optional, see TSX_MEM_HOST. */
int  tsx_host_register(void* p, size_t bytes);
int  tsx_host_unregister(void* p);

/* ---- the hot path -------------------------------------------------------------------------- */
/* Upper bound of the transformed size of an n-byte chunk: ZSTD_compressBound(n) if compressing,
 * +28 (IV 12 + tag 16, EncryptionChunkEnumeration.java:82-84) if encrypting. */
size_t tsx_transformed_bound(size_t n, uint32_t flags);

/* Forward chain over a batch of n chunks: [Zstd frame] -> [IV||AES-256-GCM(C)||TAG], CRC32C(original).
 * Replaces CompressionChunkEnumeration.nextElement + EncryptionChunkEnumeration.nextElement for the
 * whole batch.  src_size / dst_size are the sizes of the caller's buffers: a descriptor whose [src_off, src_off + src_len) or
 * [dst_off, dst_off + dst_cap) reaches beyond them fails the call with TSX_E_INVAL before anything is touched (ABI 3; the chunk
 * bounds of the reference are the array lengths of its byte[] chunks).  ctx == NULL borrows a pooled context: on the device the calling thread chose with tsx_set_thread_device(),
 * else on the initialised device with the fewest batches in flight (one JVM drives all GPUs of the node from >= 10 RLM
 * threads, README.md:218-222). */
int tsx_transform_batch(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n,
                        const void* src, size_t src_size, void* dst, size_t dst_size, int mem_kind);

/* ---- TSX_VALIDATE_RECORDS over several calls: a segment streamed in batches ---------------------
 * The state of one stream between two calls: 192 bytes of plain memory that the CALLER owns - no pointers inside, it may be copied or
 * moved, and it belongs to no context (consecutive calls may use different contexts, or the pool). */
#define TSX_RECORDS_STATE_BYTES 192
typedef struct tsx_records_state { uint64_t opaque[24]; } tsx_records_state;

/* Begins a stream of stream_bytes bytes in all - the segment's size, which the broker knows (segmentSizeInBytes) before it reads the
 * first chunk.  TSX_E_INVAL: st == NULL. */
int tsx_records_begin(tsx_records_state* st, uint64_t stream_bytes);

/* tsx_transform_batch in every respect - every mem_kind, ctx == NULL from the pool, every chain - except that the call's chunks CONTINUE
 * the stream st describes instead of being a stream of their own.
 *   - params->flags must contain TSX_VALIDATE_RECORDS, else TSX_E_INVAL.
 *   - params->flags with TSX_VALIDATE_FRAMES: TSX_E_UNSUPPORTED before anything is touched - a batch that is open across two calls
 *     cannot have its records walked without buffering it, which is not built.  The state stays bit for bit.
 *   - bytes consumed so far + the call's src_len sum > the declared length: TSX_E_INVAL before anything is touched.
 *   - every number in the state is checked on entry (carried header bytes <= 60, consumed <= declared, the open batch's end <= declared,
 *     ...): a state that was never begun, or a damaged one, is TSX_E_INVAL.  A length yields a verdict, never an address.
 *   - on any negative return the state is as it was, bit for bit; a call with n == 0, or with only empty chunks, changes nothing.
 * Same walk, same verdict: for every stream S and every cut of S into calls and chunks, tsx_records_result after the last call reports
 * the batches, compressed_batches, first_bad_pos and first_bad_reason that ONE call over S would.  The declared length makes that
 * possible: "fewer than 61 bytes left" and "the batch reaches beyond the stream's end" are decided against it, in ensureValid()'s order,
 * as soon as a batch's 61 header bytes have arrived.
 * Carried from call to call: a header whose first 61 bytes have not all arrived, raw (at most 60 bytes, over as many tiny calls as it
 * takes); or a batch whose header has passed its checks and whose end lies behind the call's end - its position, the CRC field it expects,
 * the bytes still to come and the raw CRC32C register over its bytes from offset 21 to the call's end.  Such an open batch may span
 * several whole calls.
 * Where the verdict lands: let d be the last byte the verdict needs - bad_pos itself for "fewer than 61 bytes left"; bad_pos + 60 for
 * length, beyond-the-stream and magic; the batch's last byte for CRC.  The verdict falls in the call that holds byte d.  Earlier calls
 * have been delivered TSX_OK (an all-or-nothing upload discards them).  In that call the chunk that holds stream position
 * max(bad_pos, the call's first position) and every chunk behind it get TSX_E_RECORDS and dst_len 0; the chunks in front of it are
 * delivered; a chunk that already carries another error keeps it.  Every LATER call on that state gets TSX_E_RECORDS on every chunk, with
 * nothing allocated or launched.
 * "No chunk is reported TSX_OK whose bytes the validator has not covered" holds in this sense: the bytes of an open batch are covered
 * when the batch closes, and a stream whose tsx_records_result never reaches 1 has NOT been validated - the caller must ask.  When the
 * validator finds no memory the call returns TSX_E_NOMEM (the state stays, the call may be repeated).
 * A stream given in ONE call, with the declared length equal to the call's bytes, yields the statuses, bytes and info of
 * tsx_transform_batch with the flag. */
int tsx_transform_batch_stream(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n,
                               const void* src, size_t src_size, void* dst, size_t dst_size, int mem_kind,
                               tsx_records_state* st);

/* 1: the stream is complete (the bytes consumed equal the declared length); 0: not yet; TSX_E_INVAL: a state that was never begun (or
 * out == NULL).  In the 0 and 1 cases *out describes the stream so far: repaired_chunks summed over the calls, ms that of the last call. */
int tsx_records_result(const tsx_records_state* st, tsx_records_info* out);

/* Inverse chain: [verify tag + AES-256-GCM decrypt] -> [Zstd decode], CRC32C(restored).
 * Replaces DecryptionChunkEnumeration.nextElement + DecompressionChunkEnumeration.nextElement. */
int tsx_detransform_batch(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n,
                          const void* src, size_t src_size, void* dst, size_t dst_size, int mem_kind);

/* CRC32C only (BASELINE.json configs[1]); equals java.util.zip.CRC32C over each chunk. */
int tsx_crc32c_batch(tsx_ctx* ctx, tsx_chunk_desc* descs, uint32_t n, const void* src, size_t src_size, int mem_kind);

/* ---- device memory helpers for hosts that do not link HIP themselves (the JNI shim) --------- */
int tsx_device_malloc(int device_index, size_t bytes, void** out);
int tsx_device_free(int device_index, void* p);
int tsx_memcpy_h2d(int device_index, void* dst_dev, const void* src_host, size_t bytes);
int tsx_memcpy_d2h(int device_index, void* dst_host, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* TSXFORM_H */
