// The three stages of speculative sample groups, one by one, over files (on the GPU).
//
// tests/test_gpu_ssg.py checks grouped renders end to end; this program runs ssg_guess_kernel, ssg_load /
// ssg_finish and ssg_fold_kernel -- the shipped text: it includes the kernel's own headers in the kernel's
// order and is built with the kernel's code-generation flags (Makefile, HIPCODEGEN) into
// pathtracercuda_amd/lib/ssg_stages -- on a toy sample stream ("a sample that starts at draw-pair offset o of
// pixel p takes len(p, o) pairs and returns colour(p, o)", tests/ssg_model.py), so that
// tests/test_gpu_ssg_stages.py can compare every word with the model's and with the serial truth.
//
//   ssg_stages DIR OP [OP ...]
//
// DIR/case.hdr holds 13 little-endian 32-bit words: width, rows, ssgTiles, G, spp, chunks, ignoreFirst, cap,
// window words, look[0], look[1], order entries, pairs given (0: the context's default fill 2.0, -1.0, 1.0).
// Inputs (raw little-endian words; planes of rows x width pixels unless said otherwise):
//   order.in   packed tile coordinates          rng.in     6 planes        accum.in  float4 per pixel
//   toy.in     4 planes: seed, class, s0, s1    pairs.in   3 planes (if given)
// and, where a stage is to run on logs made elsewhere (each optional, else zero):
//   start.in [item][8][64]   log.in [item][cap][3][64] floats   end.in [item][cap][64] 16-bit   bits.in
//   [item][win][64] 64-bit   count.in [item][64]   fold.in 19 planes   patchlog.in, patchend.in, patchcount.in
// Operations, in the order given:
//   guess     ssg_guess_kernel -> the start records
//   lanes     one wave per item: ssg_load, camera_ray, then per sample the toy stream and ssg_finish<false>,
//             then ssgCount = sl.k (what trace_kernel does around these calls); clears the window bits first
//   patch     the same in a patch round (ssgPatch = 1: one carrier per tile from the fold words)
//   fold:R    ssg_fold_kernel, round R
//   chain:R   guess, lanes, fold:0, then (patch, fold:r) while dead ends are left, r <= R, as run_groups does;
//             dumps after every fold under the tag r
//   dump:TAG  every buffer to NAME.TAG.out
//
// Before any launch the host checks every file's size against the header, every order entry against the tile
// grid, every count against its capacity and every pixel's start offsets for order; anything inconsistent is
// refused with status 1.  Every HIP call is checked; the first error prints the call and ends the program
// with status 1 before anything else is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <string>
#include <vector>

#include "../pathtracercuda_amd/csrc/pt_math.h"
#include "../pathtracercuda_amd/csrc/pt_leaf_forms.h"
#include "../include/pt_hip.h"

using namespace pt;

namespace {

extern __shared__ float4 lds4[];

__device__ __forceinline__ float* lds_f() { return reinterpret_cast<float*>(lds4); }
#include "../pathtracercuda_amd/csrc/pt_dev_scene.h"
#include "../pathtracercuda_amd/csrc/pt_dev_walk.h"
#include "../pathtracercuda_amd/csrc/pt_dev_path.h"
#include "../pathtracercuda_amd/csrc/pt_dev_groups.h"
#include "../pathtracercuda_amd/csrc/pt_dev_fold.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ssg_stages: %s: %s\n", #call, hipGetErrorString(e_));                    \
            exit(1);                                                                                  \
        }                                                                                             \
    } while (0)

[[noreturn]] void fail(const std::string& what)
{
    fprintf(stderr, "ssg_stages: %s\n", what.c_str());
    exit(1);
}

// ---- the toy stream (tests/ssg_model.py: toy_hash, toy_len, toy_colour) ---------------------------
PT_DEV uint32_t toy_mix(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

PT_DEV uint32_t toy_len(uint32_t h, uint32_t cls, uint32_t s0, uint32_t s1, uint32_t o)
{
    uint32_t L;
    switch (cls) {
    case 0: L = 1; break;
    case 1: L = 2; break;
    case 2: L = h % 100u == 0 ? 3u : (((h >> 8) & 1u) ? 4u : 2u); break;
    case 3: L = 3; break;
    case 4: L = 6; break;
    case 5: L = 1 + h % 6u; break;
    case 6: L = 1 + ((h >> 8) & 1u); break;
    default: L = 6; break;
    }
    if (cls == 7 && o < s1 && s1 - o <= 6u) L = s1 - o;
    if (cls == 7 && o < s0 && s0 - o <= 6u) L = s0 - o;
    return L;
}

PT_DEV float toy_channel(uint32_t h, uint32_t ch)
{
    const uint32_t g = toy_mix(h + (ch + 1u) * 0x632BE5ABu);
    return __uint_as_float((g & 0x807FFFFFu) | ((115u + ((g >> 23) & 0xFFu) % 25u) << 23));
}

// One wave per item (a patch round: per tile).  The glue is trace_kernel's around ssg_load / ssg_finish,
// with tracing replaced by the toy stream.
__global__ void __launch_bounds__(64) toy_lanes_kernel(TraceParams P, const uint32_t* __restrict__ toy)
{
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    uint32_t pos = slot, grp = 0;
    if (!P.ssgPatch) {
        const uint32_t J = 2 * P.ssgG - 1;
        pos = slot / J;
        grp = slot - pos * J;
    }
    uint32_t pos2, lane2;
    size_t li;
    if (!ssg_pixel(P, (size_t)pos * 64 + lane, pos2, lane2, li)) return;
    const size_t npix = (size_t)P.rows * P.width;
    const uint32_t seed = toy[li], cls = toy[npix + li], s0 = toy[2 * npix + li], s1 = toy[3 * npix + li];
    Xorwow rng;
    PathState ps;
    SsgLane sl;
    Counters cnt;
    ssg_load(P, pos, grp, lane, li, npix, rng, ps, sl);
    const float fx = (float)(li % P.width), fy = (float)(li / P.width);
    camera_ray(P, fx, fy, rng, ps.o, ps.d);
    while (ps.alive) {
        uint32_t d0, base, stopOff;
        ssg_item_start(P, sl, lane, li, d0, base, stopOff);
        const uint32_t o = base + (((rng.d - d0) * kInvWeyl) >> 1) - 1u;    // this sample's start (its camera pair drawn)
        const uint32_t h = toy_mix(seed ^ (o * 0x9E3779B1u));
        xorwow_skip(rng, 2u * (toy_len(h, cls, s0, s1, o) - 1u));
        ps.L = mk(toy_channel(h, 0), toy_channel(h, 1), toy_channel(h, 2));
        ssg_finish<false>(P, ps, rng, fx, fy, sl, lane, li, cnt);
    }
    P.ssgCount[(size_t)sl.logItem * 64 + lane] = sl.k;
}

// ---- host ------------------------------------------------------------------------------------------
std::string dir;

bool read_file(const std::string& name, std::vector<uint8_t>& out)
{
    FILE* f = fopen((dir + "/" + name).c_str(), "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    out.clear();
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

struct Buf {
    const char* name;
    size_t bytes = 0;
    void* dev = nullptr;
    std::vector<uint8_t> host;      // what was loaded (for the host checks)
};

constexpr size_t kGuard = 4096;     // slack behind every allocation

void alloc(Buf& b, const char* name, size_t bytes, bool required, int fill = 0)
{
    b.name = name;
    b.bytes = bytes;
    CHECK(hipMalloc(&b.dev, bytes + kGuard));
    CHECK(hipMemset(b.dev, fill, bytes + kGuard));
    if (read_file(std::string(name) + ".in", b.host)) {
        if (b.host.size() != bytes)
            fail(std::string(name) + ".in: " + std::to_string(b.host.size()) + " bytes, the header asks for " + std::to_string(bytes));
        CHECK(hipMemcpy(b.dev, b.host.data(), bytes, hipMemcpyHostToDevice));
    } else if (required) {
        fail(std::string(name) + ".in missing");
    }
}

void dump(const Buf& b, const std::string& tag)
{
    std::vector<uint8_t> h(b.bytes);
    CHECK(hipMemcpy(h.data(), b.dev, b.bytes, hipMemcpyDeviceToHost));
    const std::string path = dir + "/" + b.name + "." + tag + ".out";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) fail("cannot create " + path);
    const size_t put = fwrite(h.data(), 1, h.size(), f);
    if (fclose(f) != 0 || put != h.size()) fail("short write to " + path);
}

struct Stages {
    uint32_t width, rows, tiles, G, spp, chunks, ignore, cap, win, look[2], nOrder, hasPairs;
    uint32_t J, npix, tilesX, tilesY, total, items;
    Buf order, rng, accum, toy, pairs, start, log, end, bits, count, fold, plog, pend, pcount, dead;
    TraceParams P;

    const uint32_t* words(const Buf& b) const { return reinterpret_cast<const uint32_t*>(b.host.data()); }

    // pixel of (pos, lane) as ssg_pixel maps it; false: none
    bool pixel(uint32_t pos, uint32_t lane, size_t& li) const
    {
        const uint32_t t = words(order)[pos], x = (t & 0xffffu) * 8u + (lane & 7u), y = (t >> 16) * 8u + (lane >> 3);
        li = (size_t)y * width + x;
        return x < width && y < rows;
    }

    void load()
    {
        std::vector<uint8_t> h;
        if (!read_file("case.hdr", h) || h.size() != 13 * 4) fail("case.hdr: want 13 words");
        const uint32_t* w = reinterpret_cast<const uint32_t*>(h.data());
        width = w[0]; rows = w[1]; tiles = w[2]; G = w[3]; spp = w[4]; chunks = w[5]; ignore = w[6]; cap = w[7]; win = w[8];
        look[0] = w[9]; look[1] = w[10]; nOrder = w[11]; hasPairs = w[12];
        if (width == 0 || rows == 0 || width > 1024 || rows > 1024) fail("case.hdr: image size");
        tilesX = (width + 7) / 8;
        tilesY = (rows + 7) / 8;
        if (G < 2 || G > 16 || spp == 0 || chunks == 0 || spp > 0xffffu || chunks > 0xffffu || (uint64_t)spp * chunks > 1000000u)
            fail("case.hdr: groups or sample counts");
        total = spp * chunks;
        const uint32_t n = total / G;
        if (cap == 0 || cap != std::min<uint32_t>({total, 2 * n + 64, 10000u})) fail("case.hdr: cap is not the plan's");
        if (win != ssg_window_words(G, n)) fail("case.hdr: window words are not the plan's");
        if (ignore > 1 || look[0] > 0xffffu || look[1] > 0xffffu) fail("case.hdr: ignoreFirst or look-back");
        if (tiles == 0 || tiles > nOrder || nOrder > tilesX * tilesY) fail("case.hdr: ssgTiles beyond the order");
        J = 2 * G - 1;
        npix = width * rows;
        items = tiles * J;
        alloc(order, "order", 4 * (size_t)nOrder, true);
        for (uint32_t i = 0; i < nOrder; ++i)
            if ((words(order)[i] & 0xffffu) >= tilesX || (words(order)[i] >> 16) >= tilesY) fail("order.in: entry beyond the tile grid");
        alloc(rng, "rng", 24 * (size_t)npix, true);
        alloc(accum, "accum", 16 * (size_t)npix, true);
        alloc(toy, "toy", 16 * (size_t)npix, true);
        for (uint32_t i = 0; i < npix; ++i)
            if (words(toy)[npix + i] > 7) fail("toy.in: class beyond 7");
        alloc(pairs, "pairs", 12 * (size_t)npix, hasPairs != 0);
        if (!hasPairs) {
            if (!pairs.host.empty()) fail("pairs.in present, the header says none");
            float* p = static_cast<float*>(pairs.dev);
            CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), 0x40000000, npix));
            CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p + npix), 0xbf800000, npix));
            CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p + 2 * (size_t)npix), 0x3f800000, npix));
        }
        alloc(start, "start", (size_t)items * kStartWords * 64 * 4, false);
        alloc(log, "log", (size_t)items * cap * 3 * 64 * 4, false);
        alloc(end, "end", (size_t)items * cap * 64 * 2, false);
        alloc(bits, "bits", (size_t)items * win * 64 * 8, false);
        alloc(count, "count", (size_t)items * 64 * 4, false);
        alloc(fold, "fold", (size_t)kFoldWords * npix * 4, false);
        alloc(plog, "patchlog", (size_t)tiles * cap * 3 * 64 * 4, false);
        alloc(pend, "patchend", (size_t)tiles * cap * 64 * 2, false);
        alloc(pcount, "patchcount", (size_t)tiles * 64 * 4, false);
        alloc(dead, "dead", 4, false);
        for (const Buf* b : {&count, &pcount})
            for (size_t i = 0; i < b->host.size() / 4; ++i)
                if (words(*b)[i] > cap) fail(std::string(b->name) + ".in: count beyond cap");
        if (!start.host.empty()) check_start();
        if (!fold.host.empty())
            for (uint32_t i = 0; i < npix; ++i)
                if (words(fold)[F_DONE * npix + i] > total) fail("fold.in: done beyond total");
        memset(&P, 0, sizeof P);
        P.accum = static_cast<float4*>(accum.dev);
        P.rng = static_cast<uint32_t*>(rng.dev);
        P.width = width;
        P.height = rows;
        P.rows = rows;
        P.rowStride = 1;
        P.fwidth = (float)width;
        P.fheight = (float)rows;
        P.spp = spp;
        P.chunks = chunks;
        P.ignoreFirst = ignore;
        P.tilesX = tilesX;
        P.tilesY = tilesY;
        P.order = static_cast<const uint32_t*>(order.dev);
        P.numSlots = items;
        P.ssgG = G;
        P.ssgTiles = tiles;
        P.ssgCap = cap;
        P.ssgLog = static_cast<float*>(log.dev);
        P.ssgEnd = static_cast<uint16_t*>(end.dev);
        P.ssgStart = static_cast<const uint32_t*>(start.dev);
        P.ssgBits = static_cast<unsigned long long*>(bits.dev);
        P.ssgWin = win;
        P.ssgCount = static_cast<uint32_t*>(count.dev);
        P.ssgLook[0] = look[0];
        P.ssgLook[1] = look[1];
        P.fold = static_cast<uint32_t*>(fold.dev);
        P.cam.origin = f3{0.0f, 0.0f, 0.0f};
        P.cam.llc = f3{-1.0f, -1.0f, -1.0f};
        P.cam.horizontal = f3{2.0f, 0.0f, 0.0f};
        P.cam.vertical = f3{0.0f, 2.0f, 0.0f};
    }

    // start records a guess can have made: per pixel, phase A offsets strictly increasing in g, phase B idle
    // or one pair later
    void check_start() const
    {
        const uint32_t* s = words(start);
        for (uint32_t pos = 0; pos < tiles; ++pos)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                size_t li;
                if (!pixel(pos, lane, li)) continue;
                uint32_t prev = 0;
                for (uint32_t g = 1; g < G; ++g) {
                    const uint32_t a = s[((size_t)(pos * J + 2 * g - 1) * kStartWords) * 64 + lane];
                    const uint32_t b = s[((size_t)(pos * J + 2 * g) * kStartWords) * 64 + lane];
                    if (a <= prev || a > 0x7fffffffu || (b != 0xffffffffu && b != a + 1)) fail("start.in: records out of order");
                    prev = a;
                }
            }
    }

    unsigned pixBlocks() const { return (unsigned)(((size_t)tiles * 64 + 255) / 256); }

    void sync()
    {
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }

    void guess()
    {
        ssg_guess_kernel<<<pixBlocks(), 256, 0, 0>>>(P, static_cast<const float*>(pairs.dev), total / G,
                                                     static_cast<uint32_t*>(start.dev));
        sync();
    }

    void lanes()
    {
        CHECK(hipMemset(bits.dev, 0, bits.bytes));
        toy_lanes_kernel<<<items, 64, 0, 0>>>(P, static_cast<const uint32_t*>(toy.dev));
        sync();
    }

    void patch()
    {
        TraceParams Q = P;
        Q.ssgPatch = 1;
        Q.ssgLog = static_cast<float*>(plog.dev);
        Q.ssgEnd = static_cast<uint16_t*>(pend.dev);
        Q.ssgCount = static_cast<uint32_t*>(pcount.dev);
        Q.numSlots = tiles;
        toy_lanes_kernel<<<tiles, 64, 0, 0>>>(Q, static_cast<const uint32_t*>(toy.dev));
        sync();
    }

    uint32_t fold_round(uint32_t r)
    {
        CHECK(hipMemset(dead.dev, 0, 4));
        ssg_fold_kernel<<<pixBlocks(), 256, 0, 0>>>(P, r, static_cast<const float*>(plog.dev), static_cast<const uint16_t*>(pend.dev),
                                                    static_cast<const uint32_t*>(pcount.dev), cap, static_cast<float*>(pairs.dev),
                                                    static_cast<uint32_t*>(dead.dev));
        sync();
        uint32_t d = 0;
        CHECK(hipMemcpy(&d, dead.dev, 4, hipMemcpyDeviceToHost));
        return d;
    }

    void dump_all(const std::string& tag)
    {
        for (const Buf* b : {&rng, &accum, &pairs, &start, &log, &end, &bits, &count, &fold, &plog, &pend, &pcount, &dead}) dump(*b, tag);
    }

    void chain(uint32_t rounds)
    {
        guess();
        lanes();
        uint32_t d = fold_round(0);
        dump_all("0");
        for (uint32_t r = 1; d != 0 && r <= rounds; ++r) {
            patch();
            d = fold_round(r);
            dump_all(std::to_string(r));
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) fail("usage: ssg_stages DIR OP [OP ...]");
    dir = argv[1];
    Stages S;
    S.load();
    for (int i = 2; i < argc; ++i) {
        const std::string op = argv[i];
        const size_t colon = op.find(':');
        const std::string head = op.substr(0, colon), arg = colon == std::string::npos ? "" : op.substr(colon + 1);
        if (head == "guess" && arg.empty()) S.guess();
        else if (head == "lanes" && arg.empty()) S.lanes();
        else if (head == "patch" && arg.empty()) S.patch();
        else if (head == "fold" && !arg.empty() && arg.size() < 3) S.fold_round((uint32_t)atoi(arg.c_str()));
        else if (head == "chain" && !arg.empty() && arg.size() < 3) S.chain((uint32_t)atoi(arg.c_str()));
        else if (head == "dump" && !arg.empty()) S.dump_all(arg);
        else fail("unknown operation " + op);
    }
    printf("ssg_stages: %d operations done\n", argc - 2);
    return 0;
}
