// PNG encoding of image batches on the GPU: the lossless counterpart of jpeg_enc.hip (the inference scripts keep commented '.png'
// variants of their writers, and lossless files are what python -m wu.fid wants: JPEG artefacts bias the statistic).
//
// 8-bit RGB, colour type 2, no interlace, no ancillary chunks.  For photographs most of PNG's compression comes from the row filters
// and Huffman coding, not from LZ77 matching, and filter + literal-only deflate is parallel from end to end.  Three launches for a
// whole batch whatever N and the image sizes:
//   1. filter: one workgroup per row.  The five filter residuals (None, Sub, Up, Average, Paeth; bpp = 3, the prior row of row 0 is
//      zeros) straight from the samples (u8 / f32 / bf16 through arbitrary element strides), cost_t = sum of min(r, 256 - r), the
//      cheapest type (ties: the smallest type number), the filtered row -- type byte, then residuals -- into the workspace.
//   2. deflate: one workgroup per 32 KiB segment of an image's filtered stream.  Histogram in LDS, length-limited (<= 15) Huffman code
//      lengths and canonical codes, the run-length-coded code-length alphabet, one literal-only dynamic block packed LSB-first in LDS
//      -- or one stored block where that is not larger -- into the segment's slot; Adler-32 partial sums of the segment.
//   3. frame: one workgroup per segment.  Offsets from the segment sizes, one IDAT chunk per segment with its CRC-32 (per-thread
//      CRCs combined by multiplication with x^(8 n) mod P), zlib header 78 01 in the first, Adler-32 in the last; signature, IHDR,
//      IEND and the byte count by the first segment's workgroup.
//
// With WU_PNG_ENC_LZ77 (wu_png_enc_encode_ex) two more launches follow the deflate kernel -- 2b below: per segment a data-parallel
// LZ77 match and parse, and a block of literals and matches that replaces the segment's block only where it is strictly smaller.
//
// Every segment but the last ends with an empty stored block (the sync-flush marker, as pigz writes it), so every segment starts on a
// byte boundary and compaction is a byte copy: at most 5 bytes per 32 KiB.  A stored segment takes its bytes + 5, so a file never
// exceeds wu_png_enc_out_stride: no overflow, no fallback.
//
// Code construction (restated line by line in tests/_png_enc_ref.py): symbols in use sorted by (count, symbol); Huffman's algorithm on
// two queues, a leaf winning a tie against an internal node; only the NUMBER of codes per length is taken from the tree (lengths over
// the limit folded back as zlib's gen_bitlen does), and the lengths go to the symbols in sorted order, longest first.  Literals and
// end-of-block always give two symbols or more, so the code is complete; the single distance code has length 1 (RFC 1951 3.2.7).
//
// WU_PNG_ENC_EMU: scratch/png_lz_emu.cpp includes this file as host C++ with the few HIP names the segment kernels use defined by
// itself (256 host threads and a barrier per workgroup), and runs deflate, match and coding under the address and undefined-behaviour
// sanitizers against the restatement's bytes.  The filter, the frame and the host entry points are left out of that build.
#ifndef WU_PNG_ENC_EMU
#include "codec_internal.h"
#include "png_internal.h"
#endif

namespace {

constexpr int kSeg = kPngSeg;              // filtered bytes per deflate block
constexpr int kSlot = kSeg + 16;           // bytes of a segment's slot: at most kSeg + 5 are used
constexpr int kPer = kSeg / 256;           // bytes per thread of the deflate kernel
constexpr int kLit = 257;                  // literals and end-of-block
constexpr int kSeqLen = 258;               // code lengths sent: 257 literal/length codes, 1 distance code
constexpr int kFrameFixed = 8 + 25 + 2 + 4 + 12;       // signature, IHDR, zlib header, Adler-32, IEND

struct PngEncDesc {            // 16 bytes per image, built by the caller
    int h, w;
    int pad0, pad1;
};

struct Geo {
    int h, w, nseg;
    long long row, len;        // bytes of a filtered row (1 + 3 w) and of the filtered stream
};
__host__ __device__ __forceinline__ Geo make_geo(int h, int w, int Hmax, int Wmax) {
    Geo g;
    g.h = h < 1 ? 1 : (h > Hmax ? Hmax : h);      // clamped to the batch bounds: a bad descriptor cannot make a kernel leave its buffers
    g.w = w < 1 ? 1 : (w > Wmax ? Wmax : w);
    g.row = 1 + 3ll * g.w;
    g.len = g.row * g.h;
    g.nseg = (int)((g.len + kSeg - 1) / kSeg);
    return g;
}

#ifndef WU_PNG_ENC_EMU
// ---- 1. filter ------------------------------------------------------------------------------------------------------------------------
// x: the byte, a: left (3 bytes back), b: above, c: above left
__device__ __forceinline__ void residuals(int x, int a, int b, int c, int* r) {
    r[0] = x;
    r[1] = (x - a) & 255;
    r[2] = (x - b) & 255;
    r[3] = (x - ((a + b) >> 1)) & 255;
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    r[4] = (x - ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c))) & 255;
}

template <int DT>
__device__ __forceinline__ void fetch_xabc(const void* __restrict__ src, long long base, long long sy, long long sc, long long sx, int y, int i,
                                           int* r) {
    const int px = i / 3, ch = i - 3 * px;
    const long long at = base + (long long)px * sx + (long long)ch * sc;
    const int x = load_byte<DT>(src, at);
    const int a = px > 0 ? load_byte<DT>(src, at - sx) : 0;
    const int b = y > 0 ? load_byte<DT>(src, at - sy) : 0;
    const int c = (px > 0 && y > 0) ? load_byte<DT>(src, at - sy - sx) : 0;
    residuals(x, a, b, c, r);
}

template <int DT>
__global__ __launch_bounds__(256) void png_enc_filter_kernel(const void* __restrict__ src, long long sn, long long sc, long long sy,
                                                             long long sx, const PngEncDesc* __restrict__ desc, uint8_t* __restrict__ filt,
                                                             long long fstride, int Hmax, int Wmax) {
    __shared__ unsigned scost[5];
    const int y = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    if (y >= g.h) return;
    if (tid < 5) scost[tid] = 0u;
    __syncthreads();
    const int nb = 3 * g.w;
    const long long base = (long long)n * sn + (long long)y * sy;
    unsigned cost[5] = {0u, 0u, 0u, 0u, 0u};
    for (int i = tid; i < nb; i += 256) {
        int r[5];
        fetch_xabc<DT>(src, base, sy, sc, sx, y, i, r);
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += (unsigned)min(r[t], 256 - r[t]);
    }
#pragma unroll
    for (int t = 0; t < 5; ++t)
        if (cost[t]) atomicAdd(&scost[t], cost[t]);
    __syncthreads();
    int best = 0;
#pragma unroll
    for (int t = 1; t < 5; ++t)
        if (scost[t] < scost[best]) best = t;                          // ties: the smallest type number
    uint8_t* out = filt + (long long)n * fstride + (long long)y * g.row;
    if (tid == 0) out[0] = (uint8_t)best;
    for (int i = tid; i < nb; i += 256) {
        int r[5];
        fetch_xabc<DT>(src, base, sy, sc, sx, y, i, r);
        out[1 + i] = (uint8_t)r[best];
    }
}

#endif  // WU_PNG_ENC_EMU

// ---- Huffman code construction ------------------------------------------------------------------------------------------------------------
struct CodeScratch {
    uint32_t wt[2 * 288];      // node weights: the leaves in sorted order, then the internal nodes in the order they are made
    uint16_t parent[2 * 288];
    uint16_t order[288];       // symbols in use, by (count, symbol)
    uint8_t depth[2 * 288];
    int blc[16];               // codes per length
    int m;                     // symbols in use
};

// Lengths (<= maxbits) and bit-reversed canonical codes of the n symbols counted in `freq`, by the whole workgroup.  Ends in a barrier.
__device__ void build_code(const uint32_t* freq, int n, int maxbits, uint8_t* lens, uint16_t* codes, CodeScratch& s, int tid) {
    for (int sym = tid; sym < n; sym += 256) {
        const uint32_t f = freq[sym];
        lens[sym] = 0;
        if (f) {
            int r = 0;
            for (int t = 0; t < n; ++t) {
                const uint32_t ft = freq[t];
                r += (ft && (ft < f || (ft == f && t < sym))) ? 1 : 0;
            }
            s.order[r] = (uint16_t)sym;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int t = 0; t < n; ++t) m += freq[t] ? 1 : 0;
        s.m = m;
        for (int b = 0; b < 16; ++b) s.blc[b] = 0;
        if (m == 1) {
            s.blc[1] = 1;
        } else if (m > 1) {
            for (int i = 0; i < m; ++i) s.wt[i] = freq[s.order[i]];
            int i = 0, j = m;
            for (int k = m; k < 2 * m - 1; ++k) {                        // two queues: leaves [i, m), internal nodes [j, k)
                const int a = (i < m && (j >= k || s.wt[i] <= s.wt[j])) ? i++ : j++;
                const int b = (i < m && (j >= k || s.wt[i] <= s.wt[j])) ? i++ : j++;
                s.wt[k] = s.wt[a] + s.wt[b];
                s.parent[a] = s.parent[b] = (uint16_t)k;
            }
            s.depth[2 * m - 2] = 0;
            for (int k = 2 * m - 3; k >= m; --k) s.depth[k] = (uint8_t)(s.depth[s.parent[k]] + 1);
            int overflow = 0;                                            // nodes below the limit, internal ones included (gen_bitlen)
            for (int k = m; k < 2 * m - 2; ++k) overflow += s.depth[k] > maxbits ? 1 : 0;
            for (int l = 0; l < m; ++l) {
                int dpt = s.depth[s.parent[l]] + 1;
                if (dpt > maxbits) { dpt = maxbits; ++overflow; }
                ++s.blc[dpt];
            }
            while (overflow > 0) {                                       // zlib's gen_bitlen: move one leaf down, two overflowed ones up
                int bits = maxbits - 1;
                while (bits > 1 && s.blc[bits] == 0) --bits;             // the guard is never reached: there are fewer symbols than 2^maxbits
                --s.blc[bits];
                s.blc[bits + 1] += 2;
                --s.blc[maxbits];
                overflow -= 2;
            }
        }
    }
    __syncthreads();
    const int m = s.m;
    for (int i = tid; i < m; i += 256) {                                 // the rarest symbols take the longest codes
        int acc = 0, len = 0;
        for (int b = maxbits; b >= 1; --b) {
            acc += s.blc[b];
            if (i < acc) { len = b; break; }
        }
        lens[s.order[i]] = (uint8_t)len;
    }
    __syncthreads();
    for (int sym = tid; sym < n; sym += 256) {
        const int l = lens[sym];
        uint32_t code = 0;
        if (l) {
            for (int b = 1; b <= l; ++b) code = (code + (uint32_t)s.blc[b - 1]) << 1;        // RFC 1951 3.2.2; blc[0] = 0
            for (int t = 0; t < sym; ++t) code += lens[t] == l ? 1u : 0u;
            code = __brev(code) >> (32 - l);                             // Huffman codes go into the stream MSB first
        }
        codes[sym] = (uint16_t)code;
    }
    __syncthreads();
}

struct LsbWriter {             // LSB-first bit stream ORed into zeroed 32-bit LDS words; neighbours share edge words
    uint32_t* words;
    unsigned widx;
    unsigned long long acc;    // the low `nacc` bits are pending
    int nacc;
    __device__ __forceinline__ void start(uint32_t* w, unsigned bitpos) {
        words = w; widx = bitpos >> 5; nacc = (int)(bitpos & 31u); acc = 0ull;
    }
    __device__ __forceinline__ void put(uint32_t code, int n) {          // n <= 16
        acc |= (unsigned long long)code << nacc;
        nacc += n;
        if (nacc >= 32) {
            if ((uint32_t)acc) atomicOr(words + widx, (uint32_t)acc);
            ++widx;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0 && (uint32_t)acc) atomicOr(words + widx, (uint32_t)acc);
    }
};

// ---- 2. deflate -----------------------------------------------------------------------------------------------------------------------
// seginfo: 4 words per segment: bytes in the slot, sum of the segment's bytes mod 65521, sum of (len - j) * byte_j mod 65521, 1 = stored
__global__ __launch_bounds__(256) void png_enc_deflate_kernel(const uint8_t* __restrict__ filt, long long fstride,
                                                              const PngEncDesc* __restrict__ desc, uint8_t* __restrict__ slots,
                                                              uint32_t* __restrict__ seginfo, int nseg_max, int Hmax, int Wmax) {
    __shared__ uint32_t sout[kSlot / 4];
    __shared__ uint32_t sfreq[288];
    __shared__ uint8_t slen[288];
    __shared__ uint16_t scode[288];
    __shared__ uint32_t sclfreq[32];
    __shared__ uint8_t scllen[32];
    __shared__ uint16_t sclcode[32];
    __shared__ uint8_t stoksym[264], stokext[264];
    __shared__ CodeScratch cs;
    __shared__ unsigned sscan[256];
    __shared__ unsigned long long sadl[2];
    __shared__ int smisc[4];                                              // tokens, code-length codes sent, header bits, stored
    const int seg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    if (seg >= g.nseg) return;
    const long long segoff = (long long)seg * kSeg;
    const int len = (int)min((long long)kSeg, g.len - segoff);
    const bool last = seg == g.nseg - 1;
    const uint8_t* in = filt + (long long)n * fstride + segoff;
    uint8_t* slot = slots + ((long long)n * nseg_max + seg) * kSlot;
    for (int i = tid; i < kSlot / 4; i += 256) sout[i] = 0u;
    for (int i = tid; i < 288; i += 256) sfreq[i] = 0u;
    if (tid < 32) sclfreq[tid] = 0u;
    if (tid < 2) sadl[tid] = 0ull;
    __syncthreads();
    // this thread's kPer bytes, kept in registers for the three passes (the rows past `len` are inside the workspace and never used)
    const int first = tid * kPer;
    uint32_t wd[kPer / 4];
#pragma unroll
    for (int q = 0; q < kPer / 16; ++q) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (first + q * 16 < len) v = *(const uint4*)(in + first + q * 16);
        wd[4 * q] = v.x; wd[4 * q + 1] = v.y; wd[4 * q + 2] = v.z; wd[4 * q + 3] = v.w;
    }
    {
        uint32_t s1 = 0u, s2 = 0u;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            if (first + i < len) {
                const uint32_t b = (wd[i >> 2] >> (8 * (i & 3))) & 255u;
                atomicAdd(&sfreq[b], 1u);
                s1 += b;
                s2 += (uint32_t)(len - (first + i)) * b;                 // <= 128 * 32768 * 255
            }
        }
        if (s1) {
            atomicAdd(&sadl[0], (unsigned long long)s1);
            atomicAdd(&sadl[1], (unsigned long long)s2);
        }
        if (tid == 0) sfreq[256] = 1u;                                   // end of block
    }
    __syncthreads();
    build_code(sfreq, kLit, 15, slen, scode, cs, tid);
    unsigned bits = 0u;
#pragma unroll
    for (int i = 0; i < kPer; ++i)
        if (first + i < len) bits += slen[(wd[i >> 2] >> (8 * (i & 3))) & 255u];
    const unsigned incl = block_scan_inclusive(bits, sscan, tid);
    const unsigned litbits = sscan[255];
    if (tid == 0) {
        // the 258 code lengths, run-length coded: 18 = 11..138 zeros, 17 = 3..10 zeros, 16 = the previous length 3..6 times more
        int nt = 0, i = 0;
        auto tok = [&](int sym, int ext) { stoksym[nt] = (uint8_t)sym; stokext[nt] = (uint8_t)ext; ++nt; ++sclfreq[sym]; };
        while (i < kSeqLen) {
            const int v = i < kLit ? slen[i] : 1;
            int run = 1;
            while (i + run < kSeqLen && (i + run < kLit ? slen[i + run] : 1) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int c = min(run, 138); tok(18, c - 11); run -= c; }
                if (run >= 3) { tok(17, run - 3); run = 0; }
                while (run-- > 0) tok(0, 0);
            } else {
                tok(v, 0);
                --run;
                while (run >= 3) { const int c = min(run, 6); tok(16, c - 3); run -= c; }
                while (run-- > 0) tok(v, 0);
            }
        }
        smisc[0] = nt;
    }
    __syncthreads();
    build_code(sclfreq, 19, 7, scllen, sclcode, cs, tid);
    if (tid == 0) {
        int ncl = 19;
        while (ncl > 4 && scllen[kClOrder[ncl - 1]] == 0) --ncl;
        unsigned hb = 3 + 5 + 5 + 4 + 3 * ncl;
        for (int t = 0; t < smisc[0]; ++t) {
            const int sym = stoksym[t];
            hb += scllen[sym] + (sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)));
        }
        const unsigned total = hb + litbits + slen[256];
        const unsigned dyn = last ? (total + 7) >> 3 : ((total + 3 + 7) >> 3) + 4;
        smisc[1] = ncl;
        smisc[2] = (int)hb;
        smisc[3] = (unsigned)len + 5u <= dyn ? 1 : 0;                    // stored where that is not larger
    }
    __syncthreads();
    const bool stored = smisc[3] != 0;
    const unsigned hb = (unsigned)smisc[2], total = hb + litbits + slen[256];
    unsigned nbytes;
    if (stored) {
        nbytes = (unsigned)len + 5u;
        if (tid == 0) {
            slot[0] = last ? 1 : 0;
            slot[1] = (uint8_t)(len & 255);
            slot[2] = (uint8_t)(len >> 8);
            slot[3] = (uint8_t)(~len & 255);
            slot[4] = (uint8_t)((~len >> 8) & 255);
        }
        for (int i = tid; i < len; i += 256) slot[5 + i] = in[i];
    } else {
        nbytes = last ? (total + 7) >> 3 : ((total + 3 + 7) >> 3) + 4;
        LsbWriter bw;
        if (tid == 0) {
            bw.start(sout, 0u);
            bw.put(last ? 1u : 0u, 1);
            bw.put(2u, 2);                                               // dynamic Huffman
            bw.put(0u, 5);                                               // HLIT: 257 codes
            bw.put(0u, 5);                                               // HDIST: 1 code
            bw.put((uint32_t)(smisc[1] - 4), 4);
            for (int k = 0; k < smisc[1]; ++k) bw.put(scllen[kClOrder[k]], 3);
            for (int t = 0; t < smisc[0]; ++t) {
                const int sym = stoksym[t];
                bw.put(sclcode[sym], scllen[sym]);
                if (sym >= 16) bw.put(stokext[t], sym == 16 ? 2 : (sym == 17 ? 3 : 7));
            }
            bw.finish();
            bw.start(sout, hb + litbits);
            bw.put(scode[256], slen[256]);
            bw.finish();
            if (!last) {                                                 // empty stored block: 000, pad to a byte, 00 00 FF FF
                const unsigned at = ((total + 3 + 7) >> 3) + 2;
                atomicOr(&sout[at >> 2], 0xFFu << (8 * (at & 3)));
                atomicOr(&sout[(at + 1) >> 2], 0xFFu << (8 * ((at + 1) & 3)));
            }
        }
        if (bits) {
            bw.start(sout, hb + incl - bits);
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                if (first + i < len) {
                    const uint32_t b = (wd[i >> 2] >> (8 * (i & 3))) & 255u;
                    bw.put(scode[b], slen[b]);
                }
            }
            bw.finish();
        }
        __syncthreads();
        for (unsigned i = tid; i < (nbytes + 3) >> 2; i += 256) ((uint32_t*)slot)[i] = sout[i];
    }
    if (tid == 0) {
        uint32_t* info = seginfo + ((long long)n * nseg_max + seg) * 4;
        info[0] = nbytes;
        info[1] = (uint32_t)(sadl[0] % kAdlerMod);
        info[2] = (uint32_t)(sadl[1] % kAdlerMod);
        info[3] = stored ? 1u : 0u;
    }
}

// ---- 2b. LZ77 matching (WU_PNG_ENC_LZ77; restated in tests/_png_lz_ref.py) --------------------------------------------------------------
// Two more launches between deflate and frame, one workgroup per segment each.  The deflate kernel above has already written the
// smaller of the stored and the literal-only block; the LZ77 block replaces it only where it is strictly smaller, so a segment
// without a useful match stays byte for byte what it was and no file grows.
//
// The rule.  Hash of the three bytes at p: ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1) >> 19.  The segment is walked in blocks of 64
// positions (one wave of the workgroup in turn): every position of a block reads the head table at its hash, barrier, the block is
// inserted with atomicMax (the largest position of a hash stays, whatever the order), barrier: at most 512 rounds.  Candidates of p,
// in this order: the distances 1, 3, rowstride - 3, rowstride, rowstride + 3 (rowstride = 1 + 3 w), then the head candidate;
// distances outside [1, p] are skipped, so nothing reaches in front of the segment.  Each is extended to at most min(258, n - p)
// bytes; the longest wins, a tie goes to the earlier candidate, under 3 bytes is no match.  One lazy step: a match at p is dropped
// (p becomes a literal) where the match found at p + 1 is longer.  The parse is greedy from position 0: next[p] = p + max(len, 1).
//
// The parse without a 32768-step walk: a thread owns 128 consecutive positions.  Backwards over them it turns next[p] into "where
// the walk that enters at p leaves my chunk" (128 steps, its own positions only); one thread then hops from chunk to chunk (at most
// 256 steps) and notes where the walk enters each; every thread walks its chunk from there (at most 128 steps) and flags the
// positions where a token starts.  Every loop is bounded before it starts.
//
// Words of the token array (32768 per segment, in the workspace): bit 31 = a token starts here, bits 16..24 = match length (0: a
// literal, then bits 0..7 = the byte), bits 0..14 = distance.
constexpr int kLzBlock = 64;               // positions that read the head table before any of them is inserted: one wave
constexpr int kLzHashBits = 13;
constexpr int kLzMin = 3, kLzMax = 258;
constexpr int kLzChunk = kSeg / 256;       // positions per thread in the parse and in the coding kernel
constexpr uint32_t kLzTok = 0x80000000u;
constexpr int kLzLit = 286, kLzDist = 30;  // literal/length and distance symbols
static_assert(kLzChunk == 128 && kSeg <= 65535 && ((1 << kLzHashBits) + kSeg / 4) * 4 >= 2 * kSeg, "positions and next[] fit 16 bits; the exits fit the dead LDS");

__device__ __forceinline__ uint32_t lz_hash(uint32_t b0, uint32_t b1, uint32_t b2) {
    return ((b0 | (b1 << 8) | (b2 << 16)) * 0x9E3779B1u) >> (32 - kLzHashBits);
}
// the four bytes from byte i on, from two aligned words (one ds_read2_b32): reads the word behind the one i lies in
__device__ __forceinline__ uint32_t lz_word(const uint32_t* s, int i) {
    const unsigned long long two = (unsigned long long)s[i >> 2] | ((unsigned long long)s[(i >> 2) + 1] << 32);
    return (uint32_t)(two >> (8 * (i & 3)));
}
// bytes that agree from p and from c on, at most `limit` (<= 258); reads at most 7 bytes past p + limit - 1
__device__ __forceinline__ int lz_extend(const uint32_t* s, int p, int c, int limit) {
    int l = 0;
    for (int it = 0; it < (kLzMax + 3) / 4 && l < limit; ++it) {
        const uint32_t x = lz_word(s, p + l) ^ lz_word(s, c + l);
        if (x) { l += (__ffs((int)x) - 1) >> 3; break; }
        l += 4;
    }
    return min(l, limit);
}

__global__ __launch_bounds__(256) void png_enc_match_kernel(const uint8_t* __restrict__ filt, long long fstride,
                                                            const PngEncDesc* __restrict__ desc, uint32_t* __restrict__ toks, int nseg_max,
                                                            int Hmax, int Wmax) {
    // head table (1 + the largest inserted position of a hash, 0 = none), then the segment with zeros behind it; once the matches are
    // found both are dead and the parse keeps its chunk exits there
    __shared__ uint32_t sbig[(1 << kLzHashBits) + kSeg / 4 + 4];
    __shared__ uint16_t snxt[kSeg];                                       // head candidates, then match lengths, then next[]
    __shared__ int sentry[256];
    const int seg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    if (seg >= g.nseg) return;
    const long long segoff = (long long)seg * kSeg;
    const int len = (int)min((long long)kSeg, g.len - segoff);
    const uint8_t* in = filt + (long long)n * fstride + segoff;
    uint32_t* m = toks + ((long long)n * nseg_max + seg) * kSeg;
    uint32_t* shead = sbig;
    uint32_t* sbytes = sbig + (1 << kLzHashBits);
    const uint8_t* s = (const uint8_t*)sbytes;
    uint16_t* nxt = snxt;
    uint16_t* ex = (uint16_t*)sbig;                                       // kSeg entries
    for (int i = tid; i < (1 << kLzHashBits); i += 256) shead[i] = 0u;
    for (int i = tid; i < kSeg / 4 + 4; i += 256) {
        const int keep = len - 4 * i;
        uint32_t w = 0u;
        if (keep > 0) {
            w = ((const uint32_t*)in)[i];                                 // whole segments lie inside the workspace
            if (keep < 4) w &= (1u << (8 * keep)) - 1u;
        }
        sbytes[i] = w;
    }
    __syncthreads();
    // head candidates: everything in LDS, so the 1024 barriers wait for LDS only
    const int nrounds = (len + 255) / 256;                                // <= 128, four blocks each: the workgroup's waves in turn
    for (int r = 0; r < nrounds; ++r) {
        const int p = r * 256 + tid;
        const bool has = p + kLzMin <= len;
        const uint32_t h = has ? lz_hash(s[p], s[p + 1], s[p + 2]) : 0u;
        for (int w = 0; w < 256 / kLzBlock; ++w) {
            const bool mine = has && tid / kLzBlock == w;
            if (mine) nxt[p] = (uint16_t)shead[h];                        // <= 32766
            __syncthreads();
            if (mine) atomicMax(&shead[h], (uint32_t)(p + 1));
            __syncthreads();
        }
        if (p < len && !has) nxt[p] = 0;
    }
    const int rs = (int)g.row;
    const int fixed[5] = {1, 3, rs - 3, rs, rs + 3};
    for (int p = tid; p < len; p += 256) {
        const int limit = min(kLzMax, len - p);
        const int hc = nxt[p];                                            // written by this thread above
        int best = kLzMin - 1, bd = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int dist = k < 5 ? fixed[k] : (hc ? p - (hc - 1) : 0);
            if (dist < 1 || dist > p || best >= limit) continue;
            if (s[p + best] != s[p - dist + best]) continue;              // a longer match agrees there too
            const int l = lz_extend(sbytes, p, p - dist, limit);
            if (l > best) { best = l; bd = dist; }                        // a tie stays with the earlier candidate
        }
        if (best < kLzMin) { best = 0; bd = 0; }
        m[p] = ((uint32_t)best << 16) | (uint32_t)bd;
        nxt[p] = (uint16_t)best;
    }
    __syncthreads();
    for (int p = tid; p < len; p += 256)                                  // the lazy step, on the lengths as they were found
        if (nxt[p] && p + 1 < len && nxt[p + 1] > nxt[p]) m[p] = 0u;
    __syncthreads();
    for (int p = tid; p < len; p += 256) nxt[p] = (uint16_t)(p + max((int)((m[p] >> 16) & 511u), 1));       // <= len <= 32768
    __syncthreads();
    // greedy parse: where the walk leaves this thread's chunk, where it enters each chunk, which positions it visits
    const int lo = tid * kLzChunk, hi = min(len, lo + kLzChunk);
    for (int p = hi - 1; p >= lo; --p) {
        const int e = nxt[p];
        ex[p] = e < hi ? ex[e] : (uint16_t)e;
    }
    sentry[tid] = -1;
    __syncthreads();
    if (tid == 0) {
        int pos = 0;
        for (int it = 0; it < 256 && pos < len; ++it) {                   // every hop lands in a later chunk
            sentry[pos / kLzChunk] = pos;
            pos = ex[pos];
        }
    }
    __syncthreads();
    int p = sentry[tid];
    if (p >= 0) {
        for (int it = 0; it < kLzChunk && p < hi; ++it) {                 // the walk itself reads LDS only
            const int q = nxt[p];
            m[p] = kLzTok | (q - p >= kLzMin ? m[p] : (uint32_t)in[p]);
            p = q;
        }
    }
}

// RFC 1951 3.2.5: symbol, number of extra bits and their value of a match length / distance
__device__ __forceinline__ void lz_len_code(int len, int& sym, int& eb, int& ev) {
    const int l = len - kLzMin;
    if (len == kLzMax) { sym = 285; eb = 0; ev = 0; }
    else if (l < 8) { sym = 257 + l; eb = 0; ev = 0; }
    else { eb = 29 - __clz(l); sym = 261 + 4 * eb + ((l >> eb) & 3); ev = l & ((1 << eb) - 1); }
}
__device__ __forceinline__ void lz_dist_code(int dist, int& sym, int& eb, int& ev) {
    const int dd = dist - 1;
    if (dd < 4) { sym = dd; eb = 0; ev = 0; }
    else { eb = 30 - __clz(dd); sym = 2 * eb + 2 + ((dd >> eb) & 1); ev = dd & ((1 << eb) - 1); }
}
// f(word) for every token that starts in [lo, lo + kLzChunk) and before len
template <class F>
__device__ __forceinline__ void lz_for_tokens(const uint32_t* __restrict__ m, int lo, int len, F f) {
    for (int q = 0; q < kLzChunk / 4; ++q) {
        const int p = lo + 4 * q;
        if (p >= len) break;
        const uint4 v = *(const uint4*)(m + p);                           // up to 3 words behind len: inside the segment's kSeg words
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p + j < len && (w[j] & kLzTok)) f(w[j]);
    }
}

__global__ __launch_bounds__(256) void png_enc_lzcode_kernel(const uint32_t* __restrict__ toks, const PngEncDesc* __restrict__ desc,
                                                             uint8_t* __restrict__ slots, uint32_t* __restrict__ seginfo, int nseg_max, int Hmax,
                                                             int Wmax) {
    __shared__ uint32_t sout[kSlot / 4];
    __shared__ uint32_t sfreq[288], sdfreq[32];
    __shared__ uint8_t slen[288], sdlen[32];
    __shared__ uint16_t scode[288], sdcode[32];
    __shared__ uint32_t sclfreq[32];
    __shared__ uint8_t scllen[32];
    __shared__ uint16_t sclcode[32];
    __shared__ uint8_t stoksym[320], stokext[320];                        // at most 286 + 30 code lengths
    __shared__ CodeScratch cs;
    __shared__ unsigned sscan[256];
    __shared__ int smisc[8];                                              // tokens, code-length codes sent, header bits, take it, HLIT, HDIST
    const int seg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    if (seg >= g.nseg) return;
    const int len = (int)min((long long)kSeg, g.len - (long long)seg * kSeg);
    const bool last = seg == g.nseg - 1;
    const uint32_t* m = toks + ((long long)n * nseg_max + seg) * kSeg;
    uint8_t* slot = slots + ((long long)n * nseg_max + seg) * kSlot;
    uint32_t* info = seginfo + ((long long)n * nseg_max + seg) * 4;
    for (int i = tid; i < kSlot / 4; i += 256) sout[i] = 0u;
    for (int i = tid; i < 288; i += 256) sfreq[i] = 0u;
    if (tid < 32) { sdfreq[tid] = 0u; sclfreq[tid] = 0u; }
    __syncthreads();
    const int lo = tid * kLzChunk;
    lz_for_tokens(m, lo, len, [&](uint32_t v) {
        const int l = (int)((v >> 16) & 511u);
        if (l == 0) {
            atomicAdd(&sfreq[v & 255u], 1u);
        } else {
            int sym, eb, ev;
            lz_len_code(l, sym, eb, ev);
            atomicAdd(&sfreq[sym], 1u);
            lz_dist_code((int)(v & 32767u), sym, eb, ev);
            atomicAdd(&sdfreq[sym], 1u);
        }
    });
    if (tid == 0) sfreq[256] = 1u;                                        // end of block
    __syncthreads();
    build_code(sfreq, kLzLit, 15, slen, scode, cs, tid);
    build_code(sdfreq, kLzDist, 15, sdlen, sdcode, cs, tid);
    if (tid == 0 && cs.m == 0) sdlen[0] = 1;                              // no distance in use: one code of length 1, as in the literal-only block
    __syncthreads();
    unsigned bits = 0u;
    lz_for_tokens(m, lo, len, [&](uint32_t v) {
        const int l = (int)((v >> 16) & 511u);
        if (l == 0) {
            bits += slen[v & 255u];
        } else {
            int sym, eb, ev;
            lz_len_code(l, sym, eb, ev);
            bits += slen[sym] + eb;
            lz_dist_code((int)(v & 32767u), sym, eb, ev);
            bits += sdlen[sym] + eb;
        }
    });
    const unsigned incl = block_scan_inclusive(bits, sscan, tid);
    const unsigned tokbits = sscan[255];
    if (tid == 0) {
        int hlit = kLzLit, hdist = kLzDist;
        while (hlit > 257 && slen[hlit - 1] == 0) --hlit;
        while (hdist > 1 && sdlen[hdist - 1] == 0) --hdist;
        const int nseq = hlit + hdist;
        auto at = [&](int i) { return i < hlit ? (int)slen[i] : (int)sdlen[i - hlit]; };
        // the code lengths of both codes as one sequence, run-length coded as in the literal-only block
        int nt = 0, i = 0;
        auto tok = [&](int sym, int ext) { stoksym[nt] = (uint8_t)sym; stokext[nt] = (uint8_t)ext; ++nt; ++sclfreq[sym]; };
        while (i < nseq) {
            const int v = at(i);
            int run = 1;
            while (i + run < nseq && at(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int c = min(run, 138); tok(18, c - 11); run -= c; }
                if (run >= 3) { tok(17, run - 3); run = 0; }
                while (run-- > 0) tok(0, 0);
            } else {
                tok(v, 0);
                --run;
                while (run >= 3) { const int c = min(run, 6); tok(16, c - 3); run -= c; }
                while (run-- > 0) tok(v, 0);
            }
        }
        smisc[0] = nt;
        smisc[4] = hlit;
        smisc[5] = hdist;
    }
    __syncthreads();
    build_code(sclfreq, 19, 7, scllen, sclcode, cs, tid);
    if (tid == 0) {
        int ncl = 19;
        while (ncl > 4 && scllen[kClOrder[ncl - 1]] == 0) --ncl;
        unsigned hb = 3 + 5 + 5 + 4 + 3 * ncl;
        for (int t = 0; t < smisc[0]; ++t) {
            const int sym = stoksym[t];
            hb += scllen[sym] + (sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)));
        }
        const unsigned total = hb + tokbits + slen[256];
        const unsigned nb = last ? (total + 7) >> 3 : ((total + 3 + 7) >> 3) + 4;
        smisc[1] = ncl;
        smisc[2] = (int)hb;
        smisc[3] = nb < info[0] ? 1 : 0;                                  // only where strictly smaller than stored / literal-only
    }
    __syncthreads();
    if (smisc[3] == 0) return;
    const unsigned hb = (unsigned)smisc[2], total = hb + tokbits + slen[256];
    const unsigned nbytes = last ? (total + 7) >> 3 : ((total + 3 + 7) >> 3) + 4;
    LsbWriter bw;
    if (tid == 0) {
        bw.start(sout, 0u);
        bw.put(last ? 1u : 0u, 1);
        bw.put(2u, 2);                                                   // dynamic Huffman
        bw.put((uint32_t)(smisc[4] - 257), 5);
        bw.put((uint32_t)(smisc[5] - 1), 5);
        bw.put((uint32_t)(smisc[1] - 4), 4);
        for (int k = 0; k < smisc[1]; ++k) bw.put(scllen[kClOrder[k]], 3);
        for (int t = 0; t < smisc[0]; ++t) {
            const int sym = stoksym[t];
            bw.put(sclcode[sym], scllen[sym]);
            if (sym >= 16) bw.put(stokext[t], sym == 16 ? 2 : (sym == 17 ? 3 : 7));
        }
        bw.finish();
        bw.start(sout, hb + tokbits);
        bw.put(scode[256], slen[256]);
        bw.finish();
        if (!last) {                                                     // empty stored block: 000, pad to a byte, 00 00 FF FF
            const unsigned at = ((total + 3 + 7) >> 3) + 2;
            atomicOr(&sout[at >> 2], 0xFFu << (8 * (at & 3)));
            atomicOr(&sout[(at + 1) >> 2], 0xFFu << (8 * ((at + 1) & 3)));
        }
    }
    if (bits) {
        bw.start(sout, hb + incl - bits);
        lz_for_tokens(m, lo, len, [&](uint32_t v) {
            const int l = (int)((v >> 16) & 511u);
            if (l == 0) {
                bw.put(scode[v & 255u], slen[v & 255u]);
            } else {
                int sym, eb, ev;
                lz_len_code(l, sym, eb, ev);
                bw.put(scode[sym], slen[sym]);
                bw.put((uint32_t)ev, eb);
                lz_dist_code((int)(v & 32767u), sym, eb, ev);
                bw.put(sdcode[sym], sdlen[sym]);
                bw.put((uint32_t)ev, eb);
            }
        });
        bw.finish();
    }
    __syncthreads();
    for (unsigned i = tid; i < (nbytes + 3) >> 2; i += 256) ((uint32_t*)slot)[i] = sout[i];
    if (tid == 0) {
        info[0] = nbytes;
        info[3] = 2u;                                                    // 0 literal-only, 1 stored, 2 LZ77
    }
}

#ifndef WU_PNG_ENC_EMU
// ---- 3. frame ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

__global__ __launch_bounds__(256) void png_enc_frame_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ seginfo,
                                                            int nseg_max, const PngEncDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                            long long out_stride, int* __restrict__ result, int Hmax, int Wmax) {
    __shared__ __attribute__((aligned(16))) uint8_t sv[kSlot + 16];     // the chunk from its type on: IDAT, [78 01], data, [Adler-32]
    __shared__ uint32_t stab[256];
    __shared__ uint32_t scrc;
    const int seg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    if (seg >= g.nseg) return;
    const uint32_t* info = seginfo + (long long)n * nseg_max * 4;
    long long before = 0, all = 0;
    for (int t = 0; t < g.nseg; ++t) {                                   // uniform: scalar loads
        const long long chunk = 12ll + info[4 * t] + (t == 0 ? 2 : 0) + (t == g.nseg - 1 ? 4 : 0);
        all += chunk;
        if (t < seg) before += chunk;
    }
    const bool last = seg == g.nseg - 1;
    const int sz = (int)min(info[4 * seg], (uint32_t)(kSeg + 5));
    const int head = 4 + (seg == 0 ? 2 : 0), vlen = head + sz + (last ? 4 : 0);
    stab[tid] = kCrcTab.byte[tid];
    if (tid == 0) scrc = 0u;
    const uint8_t* slot = slots + ((long long)n * nseg_max + seg) * kSlot;
    for (int i = tid; i < sz; i += 256) sv[head + i] = slot[i];
    if (tid == 0) {
        sv[0] = 'I'; sv[1] = 'D'; sv[2] = 'A'; sv[3] = 'T';
        if (seg == 0) { sv[4] = 0x78; sv[5] = 0x01; }
        if (last) {
            // Adler-32 of the filtered stream from the segments' sums: A = 1 + sum d_i, B = len + sum (len - i) d_i, mod 65521
            unsigned long long a = 1ull, b = (unsigned long long)(g.len % kAdlerMod);
            for (int t = 0; t < g.nseg; ++t) {
                const long long after = max(g.len - (long long)(t + 1) * kSeg, 0ll);
                a += info[4 * t + 1];
                b += info[4 * t + 2] + (unsigned long long)(after % kAdlerMod) * info[4 * t + 1];
                b %= kAdlerMod;
            }
            put_be32(sv + head + sz, (uint32_t)(b << 16) | (uint32_t)(a % kAdlerMod));
        }
    }
    __syncthreads();
    {
        const int per = (vlen + 255) / 256, lo = min(tid * per, vlen), hi = min(lo + per, vlen);
        const uint32_t c = crc_shift(crc_bytes(stab, sv + lo, hi - lo), (unsigned)(vlen - hi));
        if (c) atomicXor(&scrc, c);
    }
    __syncthreads();
    uint8_t* o = out + (long long)n * out_stride;
    uint8_t* p = o + 33 + before;
    for (int i = tid; i < vlen; i += 256) p[4 + i] = sv[i];
    if (tid == 0) {
        put_be32(p, (uint32_t)(vlen - 4));
        put_be32(p + 4 + vlen, scrc);
    }
    if (seg == 0 && tid == 64) {
        const uint8_t sig[16] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
        for (int i = 0; i < 16; ++i) o[i] = sig[i];
        put_be32(o + 16, (uint32_t)g.w);
        put_be32(o + 20, (uint32_t)g.h);
        o[24] = 8; o[25] = 2; o[26] = 0; o[27] = 0; o[28] = 0;           // 8 bits, RGB, deflate, adaptive filtering, no interlace
        uint32_t c = 0xFFFFFFFFu;
        for (int i = 12; i < 29; ++i) c = stab[(c ^ o[i]) & 255u] ^ (c >> 8);
        put_be32(o + 29, ~c);
        uint8_t* e = o + 33 + all;
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) e[i] = iend[i];
        result[n] = (int)(33 + all + 12);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct Layout {
    long long fstride, nseg_max, out_stride;
    size_t off_filt, off_slots, off_info, off_toks, total;
};
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool make_layout(int N, int Hmax, int Wmax, int flags, Layout& L) {
    if (flags & ~WU_PNG_ENC_LZ77) return false;
    if (N <= 0 || Hmax <= 0 || Wmax <= 0 || Hmax > 65535 || Wmax > 65535) return false;
    const Geo g = make_geo(Hmax, Wmax, Hmax, Wmax);
    if (g.len >= (1ll << 30) || g.len * N >= (1ll << 36)) return false;
    L.nseg_max = g.nseg;
    L.fstride = (long long)align256((size_t)g.nseg * kSeg);             // whole segments: the deflate kernel loads 16 bytes at a time
    L.out_stride = g.len + 5ll * g.nseg + 12ll * g.nseg + kFrameFixed;
    size_t at = 0;
    L.off_filt = at;  at = align256(at + (size_t)N * L.fstride);
    L.off_slots = at; at = align256(at + (size_t)N * L.nseg_max * kSlot);
    L.off_info = at;  at = align256(at + (size_t)N * L.nseg_max * 16);
    L.off_toks = at;                                                    // LZ77 only: one word per filtered byte of whole segments
    if (flags & WU_PNG_ENC_LZ77) at = align256(at + (size_t)N * L.nseg_max * kSeg * 4);
    L.total = at;
    return true;
}

}  // namespace

extern "C" size_t wu_png_enc_desc_bytes(void) { return sizeof(PngEncDesc); }
extern "C" size_t wu_png_enc_segment_bytes(void) { return kSeg; }

extern "C" size_t wu_png_enc_workspace_bytes(int N, int Hmax, int Wmax) {
    Layout L;
    return make_layout(N, Hmax, Wmax, 0, L) ? L.total : 0;
}

extern "C" size_t wu_png_enc_workspace_bytes_ex(int N, int Hmax, int Wmax, int flags) {
    Layout L;
    return make_layout(N, Hmax, Wmax, flags, L) ? L.total : 0;
}

extern "C" size_t wu_png_enc_seginfo_offset(int N, int Hmax, int Wmax) {
    Layout L;
    return make_layout(N, Hmax, Wmax, 0, L) ? L.off_info : 0;
}

extern "C" size_t wu_png_enc_out_stride(int Hmax, int Wmax) {
    Layout L;
    return make_layout(1, Hmax, Wmax, 0, L) ? (size_t)L.out_stride : 0;
}

extern "C" int wu_png_enc_encode_ex(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                                    void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax,
                                    int Wmax, int flags, void* stream) {
    WU_REQUIRE(src && desc_dev && workspace && out && result_dev, "png_enc_encode: null argument");
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16 || dtype == WU_PNG_ENC_U8, "png_enc_encode: dtype %d is not u8 / f32 / bf16", dtype);
    WU_REQUIRE((flags & ~WU_PNG_ENC_LZ77) == 0, "png_enc_encode: unknown flags %d", flags);
    Layout L;
    WU_REQUIRE(make_layout(N, Hmax, Wmax, flags, L), "png_enc_encode: bad shape N=%d Hmax=%d Wmax=%d", N, Hmax, Wmax);
    WU_REQUIRE(N <= 65535, "png_enc_encode: N=%d over 65535 images per batch", N);
    WU_REQUIRE(sn >= 0 && sc >= 0 && sy >= 0 && sx >= 0, "png_enc_encode: negative strides");
    WU_REQUIRE(workspace_bytes >= L.total, "png_enc_encode: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(out_bytes >= (size_t)N * L.out_stride, "png_enc_encode: output too small (%zu of %zu bytes)", out_bytes, (size_t)((size_t)N * L.out_stride));
    WU_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)desc_dev & 3) == 0 && ((uintptr_t)result_dev & 3) == 0,
               "png_enc_encode: workspace must be 256-byte aligned, descriptors / results naturally aligned");
    const int esz = dtype == WU_F32 ? 4 : (dtype == WU_BF16 ? 2 : 1);
    WU_REQUIRE(((uintptr_t)src & (esz - 1)) == 0, "png_enc_encode: source pointer not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    uint8_t* filt = ws + L.off_filt;
    uint8_t* slots = ws + L.off_slots;
    uint32_t* info = (uint32_t*)(ws + L.off_info);
    const PngEncDesc* desc = (const PngEncDesc*)desc_dev;
    const dim3 gr((unsigned)Hmax, N), gs((unsigned)L.nseg_max, N);
#define WU_PNG_FILTER(DT) hipLaunchKernelGGL(png_enc_filter_kernel<DT>, gr, dim3(256), 0, s, src, sn, sc, sy, sx, desc, filt, L.fstride, Hmax, Wmax)
    if (dtype == WU_PNG_ENC_U8) WU_PNG_FILTER(WU_PNG_ENC_U8);
    else if (dtype == WU_F32) WU_PNG_FILTER(WU_F32);
    else WU_PNG_FILTER(WU_BF16);
#undef WU_PNG_FILTER
    WU_LAUNCH_CHECK("png_enc_filter_kernel");
    hipLaunchKernelGGL(png_enc_deflate_kernel, gs, dim3(256), 0, s, filt, L.fstride, desc, slots, info, (int)L.nseg_max, Hmax, Wmax);
    WU_LAUNCH_CHECK("png_enc_deflate_kernel");
    if (flags & WU_PNG_ENC_LZ77) {
        uint32_t* toks = (uint32_t*)(ws + L.off_toks);
        hipLaunchKernelGGL(png_enc_match_kernel, gs, dim3(256), 0, s, filt, L.fstride, desc, toks, (int)L.nseg_max, Hmax, Wmax);
        WU_LAUNCH_CHECK("png_enc_match_kernel");
        hipLaunchKernelGGL(png_enc_lzcode_kernel, gs, dim3(256), 0, s, toks, desc, slots, info, (int)L.nseg_max, Hmax, Wmax);
        WU_LAUNCH_CHECK("png_enc_lzcode_kernel");
    }
    hipLaunchKernelGGL(png_enc_frame_kernel, gs, dim3(256), 0, s, slots, info, (int)L.nseg_max, desc, out, L.out_stride, result_dev, Hmax, Wmax);
    WU_LAUNCH_CHECK("png_enc_frame_kernel");
    return 0;
}

extern "C" int wu_png_enc_encode(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                                 void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax,
                                 int Wmax, void* stream) {
    return wu_png_enc_encode_ex(src, dtype, sn, sc, sy, sx, desc_dev, workspace, workspace_bytes, out, out_bytes, result_dev, N, Hmax, Wmax, 0,
                                stream);
}
#else
}  // namespace
#endif  // WU_PNG_ENC_EMU
