// Zstandard compressor, shared part (included by zstd_enc.hip, first of its stage headers; needs zstd_common.h and gcm_dev.h).
// Holds what every stage uses: lane / address-space helpers, the parser's LDS constants, the profiling macros, the format tables,
// the LDS state of a chunk (EncLds, with the aliasing rules of its members and the names of its broadcast slots), the intra-wave
// synchronisation macros, the wave reductions and wave_copy.  Nothing here touches EncLds: it only lays it out.
#define LANES 64
// "this value is the same in every lane": results of out-of-line calls and LDS broadcasts are divergent to the compiler;
// pinning the parser's state to SGPRs turns its control flow into scalar branches instead of exec-mask juggling.
#define UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x)))
// A function that is not inlined into the kernel receives generic pointers (flat_load / flat_store: both wait counters, no
// scalar base).  The parser says what it knows: its tables, the chunk and the sequence array are global memory, and their base
// addresses are the same in every lane.
#ifdef HIPEMU
#define ZS_GLOBAL
#else
#define ZS_GLOBAL __attribute__((address_space(1)))
#endif
typedef const ZS_GLOBAL uint8_t* gbytes_t;
typedef ZS_GLOBAL uint32_t* gwords_t;
struct __attribute__((packed)) zs_u64u { uint64_t v; };
struct __attribute__((packed)) zs_u32u { uint32_t v; };
__device__ static inline uint64_t gld64(gbytes_t p) { return reinterpret_cast<const ZS_GLOBAL zs_u64u*>(p)->v; }
__device__ static inline uint32_t gld32(gbytes_t p) { return reinterpret_cast<const ZS_GLOBAL zs_u32u*>(p)->v; }
__device__ static inline uint4 ld128a(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }     // 16-byte aligned
#ifdef HIPEMU
__device__ static inline void zs_put_seq(zs_seq* p, uint32_t offBase, uint32_t litLength, uint32_t mlBase, uint32_t litPos) { zs_seq q; q.offBase = offBase; q.litLength = litLength; q.mlBase = mlBase; q.litPos = litPos; *p = q; }
#else
typedef uint32_t zs_u32x4 __attribute__((ext_vector_type(4)));
__device__ static inline uint4 ld128a(gbytes_t p) { const zs_u32x4 t = *reinterpret_cast<const ZS_GLOBAL zs_u32x4*>(p); return make_uint4(t.x, t.y, t.z, t.w); }
__device__ static inline void zs_put_seq(ZS_GLOBAL zs_seq* p, uint32_t offBase, uint32_t litLength, uint32_t mlBase, uint32_t litPos) {
    zs_u32x4 t; t.x = offBase; t.y = litLength; t.z = mlBase; t.w = litPos;                    // field order of zs_seq
    *reinterpret_cast<ZS_GLOBAL zs_u32x4*>(p) = t;
}
#endif
template <class T> __device__ static inline T* uni_ptr(T* p) {
    const uint64_t a = (uint64_t)p;
    const uint32_t lo = UNI((uint32_t)a), hi = UNI((uint32_t)(a >> 32));
    return (T*)(((uint64_t)hi << 32) | lo);
}
#define ZS_RING 4096u         /* LDS source window of the parser (bytes) */
#define ZS_RWM (ZS_RING / 4 - 1)
#define ZS_FILL 2048u         /* refill granule */
#define ZS_SAFE 384u          /* the parser may touch [ip, ip + ZS_SAFE) between two refill checks */
#ifndef ZS_WAVES_PER_SIMD
#define ZS_WAVES_PER_SIMD 6   /* occupancy target: 80 VGPRs, <= 6826 B of LDS -> 24 chunks per CU */
#endif
#define ZS_SCR 1024u          /* slots of the intra-step hash-collision detector (per table) */
// cold, register-hungry scalar stages are kept out of line so the speculative match loop keeps its occupancy
#define ZS_NOINLINE __attribute__((noinline))

// ---- optional phase profile (make prof): lap timer, lane 0 attributes the cycles since the previous PT() to bucket k ----
// (make prof2 builds every source with TSX_PROF2 as well, for the decoder's light timers: here it only blanks the lap macros)
#ifdef TSX_PROF
__shared__ unsigned long long g_prof[24];
__shared__ unsigned long long g_prof_take;
static unsigned long long* g_prof_out = nullptr;                      // device buffer: 24 u64 per chunk
extern "C" void tsx_debug_set_prof(void* dev_ptr) { g_prof_out = (unsigned long long*)dev_ptr; }
#define ZS_PROF_PARAM , unsigned long long* __restrict__ prof_out     /* the service kernel's extra parameter ... */
#define ZS_PROF_ARG , prof_out                                        /* ... handed on to zstd_compress_chunk ... */
#define ZS_PROF_LAUNCH_ARG , g_prof_out                               /* ... and what the host launcher passes for it */
#else
#define ZS_PROF_PARAM
#define ZS_PROF_ARG
#define ZS_PROF_LAUNCH_ARG
#endif
#if defined(TSX_PROF) && !defined(TSX_PROF2)
#define PT(k) do { const unsigned long long now_ = (unsigned long long)clock64(); if (threadIdx.x == 0) { g_prof[k] += now_ - g_prof[23]; g_prof[23] = now_; } } while (0)
#define PCNT(k, v) do { if (threadIdx.x == 0) g_prof[k] += (v); } while (0)
#define PTW(k) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); PT(k); } while (0)   /* drain, then lap: stage latency */
#else
#define PT(k) do {} while (0)
#define PCNT(k, v) do {} while (0)
#define PTW(k) do {} while (0)
#endif

// ---- format tables ------------------------------------------------------------------------------------
__device__ static const uint8_t kLLbits[36] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,6,7,8,9,10,11,12,13,14,15,16};
__device__ static const uint8_t kMLbits[53] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,7,8,9,10,11,12,13,14,15,16};
__device__ static const short kLLdefaultNorm[36] = {4,3,2,2,2,2,2,2,2,2,2,2,2,1,1,1,2,2,2,2,2,2,2,2,2,3,2,1,1,1,1,1,-1,-1,-1,-1};
__device__ static const short kOFdefaultNorm[29] = {1,1,1,1,1,1,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1};
__device__ static const short kMLdefaultNorm[53] = {1,4,3,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1,-1,-1};
__device__ static const uint8_t kLLcode[64] = {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,16,17,17,18,18,19,19,20,20,20,20,21,21,21,21,
    22,22,22,22,22,22,22,22,23,23,23,23,23,23,23,23,24,24,24,24,24,24,24,24,24,24,24,24,24,24,24,24};
__device__ static const uint8_t kMLcode[128] = {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,
    32,32,33,33,34,34,35,35,36,36,36,36,37,37,37,37,38,38,38,38,38,38,38,38,39,39,39,39,39,39,39,39,
    40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,40,41,41,41,41,41,41,41,41,41,41,41,41,41,41,41,41,
    42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42,42};
__device__ static const uint32_t kRtb[8] = {0, 473195, 504333, 520860, 550000, 700000, 750000, 830000};

__device__ static inline uint32_t hb32(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }
__device__ static inline uint64_t ld64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ static inline uint32_t LLcode(uint32_t ll) { return ll > 63 ? hb32(ll) + 19 : kLLcode[ll]; }
__device__ static inline uint32_t MLcode(uint32_t ml) { return ml > 127 ? hb32(ml) + 36 : kMLcode[ml]; }

// ---- LDS state of one chunk (one wave per workgroup) --------------------------------------------------------
struct HufTable { uint16_t val[256]; uint8_t nb[256]; uint32_t tableLog, maxSym; };
struct FseTable { uint16_t state[512]; uint32_t dnb[56]; int32_t dfs[56]; uint32_t tableLog; };

// Slots of EncLds::scal: lane 0 writes, a barrier, every lane reads.  A slot may serve two stages that never overlap.
enum {
    ZS_SCAL_HUF_HSIZE = 0,      // compress_literals: size of the new table's description (lane 0 after huf_writeCTable -> all lanes)
    ZS_SCAL_HUF_USEOLD = 1,     // compress_literals: the previous table is cheaper than the new one with its description
    ZS_SCAL_HUF_FAIL = 2,       // compress_literals: no table can be used, the literals go out raw
    ZS_SCAL_SEQ_QOFF = 3,       // compress_sequences: where the bit stream starts behind the three table descriptions (0xFFFFFFFF: failure)
    ZS_SCAL_SEQ_COUNTSIZE = 4,  // compress_sequences: size of the last FSE description written (the "too small to be worth it" rule)
    ZS_SCAL_HUF_BC = 4,         // [4 .. 6] huf_buildCTable's three words (nonNullRank, nodeRoot, maxNbBits): the literal stage, over before [4] counts sizes
    ZS_SCAL_NEWHUF = 8,         // compress_literals sets it when it used a new table; the frame loop clears it per block and adopts huf[cur ^ 1] if the block is kept
    ZS_SCAL_MULT = 15           // frame loop, once per chunk: 10 - strategy; build_seq_table reads it (ZSTD_selectEncodingType)
};
struct EncLds {
    int hufRepeat[2];           // 0 none, 1 check
    uint32_t scal[16];          // lane-0 -> wave broadcast slots (ZS_SCAL_*)
    union alignas(16) {
        struct {                // entropy stage of a block
            // The two Huffman tables of the literal stage ([cur] = table of the previous compressed-literals block, [cur ^ 1] =
            // candidate) are dead while the sequences are coded and the LL table is dead while the literals are: they share their
            // bytes, and between two blocks the Huffman tables wait in the chunk's workspace (ZS_WS_HUFSAVE).  That is what brings
            // the wave's LDS under 160 KiB / 24: six chunks per SIMD instead of five.
            union { FseTable ll; HufTable huf[2]; };
            FseTable of;        // (the literal stage borrows it to FSE-code the Huffman weights)
            union {
                FseTable ml;            // sequence stage
                uint32_t hist[256];     // literal stage (and the pre-splitter): byte histogram, dead before ml is built
            };
            // second histogram (pre-splitter / sampling of the literals); sequence-code histograms; and, while the description of a new
            // Huffman table is written (huf_writeCTable: the sampling is over, the sequence stage has not begun), the table's weights
            // (bytes 0 .. 255) and their histogram (words 64 .. 79).  With those two arrays inside hist2 the wave's LDS is 6384 bytes: the
            // hardware allocates LDS in 1280-byte granules on gfx950, so 6704 bytes occupied 7680 and a CU held 21 chunks - not the 24 its
            // registers allow (measured: at most 5376 = 21 x 256 waves of a 6144-wave launch were ever resident at once).
            uint32_t hist2[256];
            uint8_t tableSymbol[512];
            uint16_t cumul[64];
            short norm[64];
        };
        struct {                // parse stage of a block (re-primed per block): source window + collision scoreboard
            uint32_t ring[ZS_RING / 4 + 4];     // + 16-byte mirror of the first bytes
            uint8_t scr[2 * ZS_SCR];
        } p;
        struct {                // GCM tail over the finished frame (gcm_encrypt_wave)
            tsx_gf128 tab[256];
            uint32_t t0[256];
        } g;
        uint32_t crcTab[4 * 256];       // CRC32C head over the source chunk (crc32c_wave)
    };
};

// ---- wave helpers ----------------------------------------------------------------------------------------
// Cross-lane memory hand-off inside ONE wave (lane A's store observed by lane B's later load).  The hardware issues a
// wave's vector-memory / LDS instructions in order and keeps same-address order, so nothing is needed there; the fiber
// emulator (tests/emu) does not run lanes in lockstep and needs a rendezvous.
#ifdef HIPEMU
#define WAVE_MEM_SYNC() __threadfence_block()
#define VM_DRAIN() do {} while (0)
#define LOADED64(x) do {} while (0)
#else
#define WAVE_MEM_SYNC() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)   /* compiler-level only */
#define VM_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// "this value is consumed here": pins the wait for a global load inside the branch that issued it, so that the join with
// an LDS-sourced alternative does not inherit a vmcnt(0) (which would also drain every store still in flight).
#define LOADED64(x) do { uint32_t lo_ = (uint32_t)(x), hi_ = (uint32_t)((x) >> 32); asm volatile("" : "+v"(lo_), "+v"(hi_)); (x) = ((uint64_t)hi_ << 32) | lo_; } while (0)
#endif
// The hand-off between two stages of a chunk (one wave per workgroup): every lane's earlier stores, to LDS and to global memory, are
// visible to every lane afterwards.
__device__ __forceinline__ static void stage_sync() { __threadfence_block(); __syncthreads(); }

// ---- wave-parallel pieces ---------------------------------------------------------------------------------
__device__ static inline uint32_t wave_sum(uint32_t v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ static inline uint32_t wave_max(uint32_t v) { for (int o = 32; o; o >>= 1) { uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; } return v; }
__device__ static inline uint32_t wave_excl_scan(uint32_t v, uint32_t lane) {
    uint32_t s = v;
    for (int o = 1; o < LANES; o <<= 1) { uint32_t t = __shfl_up(s, o); if (lane >= (uint32_t)o) s += t; }
    return s - v;
}
__device__ static inline void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t lane) {
    for (uint32_t i = lane; i < n; i += LANES) dst[i] = src[i];
}
// the low nbytes bytes of v, little endian (the caller is one lane): every header field of the format is written this way
__device__ __forceinline__ static void put_le(uint8_t* dst, uint64_t v, uint32_t nbytes) {
    for (uint32_t i = 0; i < nbytes; i++) dst[i] = (uint8_t)(v >> (8 * i));
}
