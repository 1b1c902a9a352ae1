// host_quant_check.cpp -- stand-alone check of the host half of the host-pointer decode path (ldpc-3gpp-matlab_amd/csrc/
// nrldpc_host_quant.cpp, compiled into this program), meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_host_quant_check.py does that).  Three parts:
//   1. nrldpc_quantise_i8_path: every path the CPU offers against path 0, for every source kind, every length 0..200 and exact-size
//      heap allocations at element offsets 0..3 (a read or write past either end is the sanitizer's to report); bytes and the -inf
//      flag must agree, with +-inf, NaN, ties and clamps at the first and last element.
//   2. the compact-row piece walk of HostPool::quantise_rows_start (nrldpc_capi.hip), restated here: for every worker count 1..16
//      over the (act, pitch, rows, lo, hi) ranges of argv[1] (the planned chunks, written by the test), every compact byte of the
//      range is written exactly once -- through nrldpc_quantise_i8 itself, into an exact-size destination -- and nothing at or beyond
//      `act` of a source row is read: those elements are poisoned for the sanitizer, and the arithmetic is checked as well.
//   3. nrldpc_top_block against a plain scan: three kinds, Z in {2, 3, 7, 20, 88}, every (cw0, cw_step) split up to 16, with blocks
//      that hold only NaN or -0.
// g++ before version 12 has no _Float16 in C++: the plain C++ path then reads halves through the conversion below, which makes
// path 0 on fp16 input a reference of its own against the F16C instructions of the other two.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <fstream>
#include <vector>

#include <sanitizer/asan_interface.h>

#if defined(__GNUC__) && !defined(__clang__) && __GNUC__ < 12
struct hq_half {
    uint16_t b;
    operator float() const {
        const uint32_t s = (uint32_t)(b & 0x8000u) << 16, e = (b >> 10) & 31u, m = b & 0x3ffu;
        float f;
        if (e == 0) f = std::ldexp((float)m, -24);
        else if (e == 31) f = m ? NAN : INFINITY;
        else f = std::ldexp((float)(m | 0x400u), (int)e - 25);
        uint32_t u;
        std::memcpy(&u, &f, 4);
        u |= s;
        std::memcpy(&f, &u, 4);
        return f;
    }
};
#define _Float16 hq_half
#endif
#include "nrldpc_host_quant.cpp"

static int fail(const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    std::fprintf(stderr, "host_quant_check: %s (%ld, %ld, %ld, %ld)\n", what, a, b, c, d);
    return 1;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint16_t f32_to_f16(float f) {  // round to nearest even; enough for the table below (no subnormal results but 0)
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(s | 0x7e00u);
    if (a >= 0x47800000u) return (uint16_t)(s | 0x7c00u);  // >= 65536 (and inf)
    if (a < 0x38800000u) return s;                          // below the smallest normal half: 0 here
    uint32_t m = a - 0x38000000u;                           // rebias
    const uint32_t lsb = (m >> 13) & 1u;
    m += 0xfffu + lsb;
    return (uint16_t)(s | (m >> 13));
}

static const float kTable[] = {0.0f, -0.0f, 0.0625f, -0.0625f, 0.1875f, -0.1875f, 0.3125f, -0.3125f, 15.875f, -15.875f, 15.9375f, -15.9375f,
                               1e4f, -1e4f, NAN, INFINITY, 1e-3f, 3.0f, -2.4375f, 7.5625f, 0.5f, -0.5f, 100.0f, -100.0f};
static const float kEdge[] = {INFINITY, -INFINITY, NAN, 0.0625f, -0.1875f, 1e4f, -1e4f, 15.9375f};

static void put(void* base, int kind, size_t i, float v) {
    if (kind == NRLDPC_HQ_F32) static_cast<float*>(base)[i] = v;
    else if (kind == NRLDPC_HQ_F64) static_cast<double*>(base)[i] = (double)v;
    else static_cast<uint16_t*>(base)[i] = f32_to_f16(v);
}

static int check_paths() {
    long compared = 0, negs = 0;
    for (int kind = 0; kind < 3; ++kind) {
        const size_t es = kind == NRLDPC_HQ_F64 ? 8 : kind == NRLDPC_HQ_F16 ? 2 : 4;
        for (size_t len = 0; len <= 200; ++len)
            for (size_t off = 0; off < 4; ++off)
                for (int edge = 0; edge < 8; ++edge) {
                    char* sbase = static_cast<char*>(std::malloc((off + len) * es + (off + len == 0)));
                    void* src = sbase + off * es;
                    for (size_t i = 0; i < len; ++i) put(src, kind, i, kTable[rnd() % (sizeof kTable / sizeof kTable[0])]);
                    if (len) {
                        put(src, kind, 0, kEdge[edge]);
                        put(src, kind, len - 1, kEdge[(edge + 1 + off) % 8]);
                    }
                    int8_t* ref = static_cast<int8_t*>(std::malloc(off + len + (off + len == 0)));
                    const bool neg0 = nrldpc_quantise_i8_path(ref + off, src, len, kind, 8.0f, 0);
                    negs += neg0;
                    for (int path = 1; path <= 2; ++path) {
                        int8_t* got = static_cast<int8_t*>(std::malloc(off + len + (off + len == 0)));
                        std::memset(got, 0x55, off + len);
                        const bool neg = nrldpc_quantise_i8_path(got + off, src, len, kind, 8.0f, path);
                        if (neg != neg0) return fail("-inf flag differs from path 0", kind, (long)len, (long)off, path);
                        if (len && std::memcmp(got + off, ref + off, len)) return fail("bytes differ from path 0", kind, (long)len, (long)off, path);
                        for (size_t i = 0; i < off; ++i)
                            if (got[i] != 0x55) return fail("write before the destination", kind, (long)len, (long)off, path);
                        std::free(got);
                        ++compared;
                    }
                    std::free(ref);
                    std::free(sbase);
                }
    }
    // the definition itself, on values whose grid value is known
    const float in[10] = {0.0625f, -0.0625f, 0.1875f, -0.1875f, 15.875f, 1e4f, -1e4f, NAN, INFINITY, -0.0f};
    const int want[10] = {0, 0, 2, -2, 127, 127, -127, 0, -128, 0};
    int8_t q[10];
    if (nrldpc_quantise_i8_path(q, in, 10, NRLDPC_HQ_F32, 8.0f, 0)) return fail("-inf reported where there is none");
    for (int i = 0; i < 10; ++i)
        if (q[i] != want[i]) return fail("grid value", i, q[i], want[i]);
    std::printf("paths ok: %ld comparisons, %ld inputs with a -inf\n", compared, negs);
    return negs ? 0 : fail("no input held a -inf");
}

// HostPool::quantise_rows_start, restated: worker w of nw over the compact range [c_lo, c_hi)
template <class F> static void walk(size_t act, size_t pitch, size_t c_lo, size_t c_hi, int w, int nw, F f) {
    const size_t n = c_hi - c_lo;
    const size_t per = ((n + nw - 1) / nw + 63) & ~(size_t)63, lo = c_lo + std::min(n, per * w), hi = std::min(c_hi, lo + per);
    for (size_t pos = lo; pos < hi;) {
        const size_t r = pos / act, in_row = pos - r * act, len = std::min(hi - pos, act - in_row);
        f(pos, r * pitch + in_row, len, in_row);
        pos += len;
    }
}

static int check_walk(const char* file) {
    std::ifstream in(file);
    int n = -1;
    in >> n;
    if (!in || n < 1) return fail("bad range file");
    long pieces = 0, crossings = 0;
    for (int t = 0; t < n; ++t) {
        size_t act, pitch, rows, lo, hi;
        int kind;
        in >> act >> pitch >> rows >> lo >> hi >> kind;
        if (!in || act > pitch || hi > rows * act || lo > hi) return fail("bad range", t);
        const size_t es = kind == NRLDPC_HQ_F64 ? 8 : kind == NRLDPC_HQ_F16 ? 2 : 4;
        // exact-size source of `rows` rows; the last row ends at `act`: nothing beyond may be touched, and what lies between act and
        // pitch of every other row is poisoned (whole 8-byte granules inside the gap)
        const size_t src_elems = (rows - 1) * pitch + act;
        char* src = static_cast<char*>(std::malloc(src_elems * es));
        for (size_t i = 0; i < src_elems; ++i) put(src, kind, i, (float)((long)(i % 31) - 15) * 0.125f);
        for (size_t r = 0; r + 1 < rows && act < pitch; ++r) {
            uintptr_t a = reinterpret_cast<uintptr_t>(src) + (r * pitch + act) * es, b = reinterpret_cast<uintptr_t>(src) + (r + 1) * pitch * es;
            a = (a + 7) & ~(uintptr_t)7;
            b &= ~(uintptr_t)7;
            if (b > a) ASAN_POISON_MEMORY_REGION(reinterpret_cast<void*>(a), b - a);
        }
        for (int nw = 1; nw <= 16; ++nw) {
            int8_t* dst = static_cast<int8_t*>(std::malloc(hi - lo));  // exact size: [lo, hi) is all that exists
            std::vector<uint8_t> hits(hi - lo, 0);
            int bad = 0;
            for (int w = 0; w < nw; ++w)
                walk(act, pitch, lo, hi, w, nw, [&](size_t pos, size_t s, size_t len, size_t in_row) {
                    if (in_row + len > act || s + len > src_elems || pos < lo || pos + len > hi) { bad = 1; return; }
                    for (size_t i = 0; i < len; ++i) ++hits[pos - lo + i];
                    (void)nrldpc_quantise_i8(dst + (pos - lo), src + s * es, len, kind, 8.0f);
                    ++pieces;
                    crossings += in_row != 0;
                });
            if (bad) return fail("a piece leaves its row or its range", t, nw);
            for (size_t i = 0; i < hi - lo; ++i) {
                if (hits[i] != 1) return fail("compact byte not written exactly once", t, nw, (long)(lo + i), hits[i]);
                const size_t pos = lo + i, r = pos / act, c = pos - r * act;
                const int want = (int)((long)((r * pitch + c) % 31) - 15);
                if (dst[i] != want) return fail("compact byte holds the wrong element", t, nw, (long)pos, dst[i]);
            }
            std::free(dst);
        }
        for (size_t r = 0; r + 1 < rows && act < pitch; ++r) {
            uintptr_t a = reinterpret_cast<uintptr_t>(src) + (r * pitch + act) * es, b = reinterpret_cast<uintptr_t>(src) + (r + 1) * pitch * es;
            a = (a + 7) & ~(uintptr_t)7;
            b &= ~(uintptr_t)7;
            if (b > a) ASAN_UNPOISON_MEMORY_REGION(reinterpret_cast<void*>(a), b - a);
        }
        std::free(src);
    }
    std::printf("walk ok: %d ranges, %ld pieces, %ld of them start inside a row\n", n, pieces, crossings);
    return 0;
}

static int check_top_block() {
    const int Zs[5] = {2, 3, 7, 20, 88};
    long calls = 0, found_nan_only = 0;
    for (int kind = 0; kind < 3; ++kind) {
        const size_t es = kind == NRLDPC_HQ_F64 ? 8 : kind == NRLDPC_HQ_F16 ? 2 : 4;
        for (int zi = 0; zi < 5; ++zi) {
            const int Z = Zs[zi], nblocks = 52, first = 14;
            for (int scene = 0; scene < 12; ++scene) {
                const size_t n_total = 1 + (size_t)(scene * 3) % 19;
                char* src = static_cast<char*>(std::calloc(n_total * nblocks * Z, es));
                int want = first - 1;
                // a few blocks that hold only NaN or -0 (they do not count), and -- in most scenes -- one real value
                for (int k = 0; k < 6; ++k) {
                    const size_t cw = rnd() % n_total, b = rnd() % nblocks;
                    for (int z = 0; z < Z; ++z) put(src, kind, (cw * nblocks + b) * Z + z, (k & 1) ? NAN : -0.0f);
                    found_nan_only += (k & 1) && (int)b >= first;
                }
                if (scene % 4 != 3)
                    for (int k = 0; k < 1 + scene % 3; ++k) {
                        const size_t cw = rnd() % n_total, b = rnd() % nblocks, z = rnd() % Z;
                        put(src, kind, (cw * nblocks + b) * Z + z, (k & 1) ? -INFINITY : 0.125f);
                        if ((int)b >= first && (int)b > want) want = (int)b;
                    }
                for (int nw = 1; nw <= 16; ++nw) {
                    int best = first - 1;
                    for (int w = nw - 1; w >= 0; --w) {  // (any order: the maximum is shared)
                        nrldpc_top_block(src, kind, n_total, (size_t)w, (size_t)nw, Z, nblocks, first, &best);
                        ++calls;
                    }
                    if (best != want) return fail("top block differs from a plain scan", kind, Z, scene, nw);
                }
                std::free(src);
            }
        }
    }
    std::printf("top_block ok: %ld calls, %ld NaN-only blocks in range\n", calls, found_nan_only);
    return found_nan_only ? 0 : fail("no NaN-only block in range");
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: host_quant_check RANGES");
    if (int rc = check_paths()) return rc;
    if (int rc = check_walk(argv[1])) return rc;
    if (int rc = check_top_block()) return rc;
    std::printf("host_quant_check ok\n");
    return 0;
}
