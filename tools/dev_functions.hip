// The trace kernel's device functions, one by one, over inputs read from files (on the GPU).
//
// tools/fp_exhaustive.hip shows that the fast forms equal the general forms ON the GPU; this program
// hands the GPU's result words out, so that tests/test_gpu_dev_functions.py can compare them with the x86
// oracle's at arguments no render produces.  It includes the headers the kernel compiles (pt_math.h,
// pt_dev_tex.h, pt_dev_tonemap.h) and is built with the kernel's code-generation flags (Makefile,
// HIPCODEGEN) into pathtracercuda_amd/lib/dev_functions.
//
//   dev_functions DIR
//
// Every file holds raw little-endian 32-bit words; a file of several arguments holds them as planes
// (all first arguments, then all second ones), results likewise.  One launch per operation, 256 threads
// per block, one input per thread.
//
//   input file        words per input   operation -> output file (words per input)
//   sincos_pos.in     x                 sincos_pos.out (sin plane, cos plane)
//   acos.in           x                 acos_.out (1), acos_sel.out (1)
//   atan2.in          y, x              atan2_.out (1), atan2_sel.out (1)
//   log.in            x                 log_.out (1)
//   exp.in            x                 exp_.out (1)
//   pow.in            x, y              pow_.out (1)
//   f2i.in            f                 f2i_x86.out (1, the int32)
//   tonemap.in        r, g, b, frames   tonemap_pixel.out (1: the four bytes r, g, b, 255)
//   tex2d.in          texture, u, v     tex2d.out (r, g, b planes); the textures come from tex2d.tab:
//                                       count, then width and height of each, then every texture's RGBA
//                                       float texels row by row.  A texture index beyond the table is
//                                       refused on the host.
//   xorwow_init.in    seed low, high    xorwow_init.out (6 per input: d, v0..v4)
//   xorwow_skip.in    low, high, draws  xorwow_skip.out (6 per input)
//   xorwow_stream.in  n, then pairs of seed low, high (NOT planes): one thread per seed draws n
//                     xorwow_next and then n uniform -> xorwow_stream.out (2 n words per seed)
//
// Every HIP call is checked; the first error prints the call and ends the program with status 1 before
// anything else is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../pathtracercuda_amd/csrc/pt_math.h"

using namespace pt;

namespace {

#include "../pathtracercuda_amd/csrc/pt_dev_tex.h"
#include "../pathtracercuda_amd/csrc/pt_dev_tonemap.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "dev_functions: %s: %s\n", #call, hipGetErrorString(e_));                 \
            exit(1);                                                                                  \
        }                                                                                             \
    } while (0)

[[noreturn]] void fail(const std::string& what)
{
    fprintf(stderr, "dev_functions: %s\n", what.c_str());
    exit(1);
}

// in: the input planes (n words each); out: the output planes; aux: the texture table (tex2d only)
#define OP_KERNEL(name) __global__ void __launch_bounds__(256) name(const uint32_t* in, uint32_t* out, uint32_t n, const DevTex* aux)
#define OP_INDEX                                                   \
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;      \
    if (!(i < n)) return;                                          \
    (void)aux

PT_DEV float fl(uint32_t w) { return __uint_as_float(w); }
PT_DEV uint32_t wd(float f) { return __float_as_uint(f); }

OP_KERNEL(k_sincos_pos)
{
    OP_INDEX;
    float s, c;
    sincos_pos(fl(in[i]), s, c);
    out[i] = wd(s);
    out[n + i] = wd(c);
}
OP_KERNEL(k_acos) { OP_INDEX; out[i] = wd(acos_(fl(in[i]))); }
OP_KERNEL(k_acos_sel) { OP_INDEX; out[i] = wd(acos_sel(fl(in[i]))); }
OP_KERNEL(k_atan2) { OP_INDEX; out[i] = wd(atan2_(fl(in[i]), fl(in[n + i]))); }
OP_KERNEL(k_atan2_sel) { OP_INDEX; out[i] = wd(atan2_sel(fl(in[i]), fl(in[n + i]))); }
OP_KERNEL(k_log) { OP_INDEX; out[i] = wd(log_(fl(in[i]))); }
OP_KERNEL(k_exp) { OP_INDEX; out[i] = wd(exp_(fl(in[i]))); }
OP_KERNEL(k_pow) { OP_INDEX; out[i] = wd(pow_(fl(in[i]), fl(in[n + i]))); }
OP_KERNEL(k_f2i) { OP_INDEX; out[i] = (uint32_t)f2i_x86(fl(in[i])); }
OP_KERNEL(k_tonemap)
{
    OP_INDEX;
    const uchar4 q = tonemap_pixel(make_float4(fl(in[i]), fl(in[n + i]), fl(in[2 * n + i]), 0.0f), in[3 * n + i]);
    out[i] = (uint32_t)q.x | ((uint32_t)q.y << 8) | ((uint32_t)q.z << 16) | ((uint32_t)q.w << 24);
}
OP_KERNEL(k_tex2d)
{
    OP_INDEX;
    const f3 c = tex2d(aux[in[i]], fl(in[n + i]), fl(in[2 * n + i]));
    out[i] = wd(c.x);
    out[n + i] = wd(c.y);
    out[2 * n + i] = wd(c.z);
}
PT_DEV void put_state(uint32_t* out, const Xorwow& s)
{
    out[0] = s.d; out[1] = s.v0; out[2] = s.v1; out[3] = s.v2; out[4] = s.v3; out[5] = s.v4;
}
OP_KERNEL(k_xorwow_init)
{
    OP_INDEX;
    put_state(out + 6 * (size_t)i, xorwow_init((uint64_t)in[i] | ((uint64_t)in[n + i] << 32)));
}
OP_KERNEL(k_xorwow_skip)
{
    OP_INDEX;
    Xorwow s = xorwow_init((uint64_t)in[i] | ((uint64_t)in[n + i] << 32));
    xorwow_skip(s, in[2 * n + i]);
    put_state(out + 6 * (size_t)i, s);
}
// in: seed pairs; n seeds; draws per seed in out's stride
__global__ void __launch_bounds__(256) k_xorwow_stream(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t draws)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!(i < n)) return;
    Xorwow s = xorwow_init((uint64_t)in[2 * i] | ((uint64_t)in[2 * i + 1] << 32));
    uint32_t* o = out + 2 * (size_t)draws * i;
    for (uint32_t k = 0; k < draws; ++k) o[k] = xorwow_next(s);
    for (uint32_t k = 0; k < draws; ++k) o[draws + k] = wd(uniform(s));
}

std::vector<uint32_t> read_words(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) fail("cannot open " + path);
    std::vector<uint32_t> w;
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    return w;
}

void write_words(const std::string& path, const std::vector<uint32_t>& w)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) fail("cannot create " + path);
    const size_t put = fwrite(w.data(), 4, w.size(), f);
    if (fclose(f) != 0 || put != w.size()) fail("short write to " + path);
}

uint32_t* to_device(const std::vector<uint32_t>& w)
{
    uint32_t* d = nullptr;
    CHECK(hipMalloc(&d, w.size() * 4));
    CHECK(hipMemcpy(d, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    return d;
}

typedef void (*OpKernel)(const uint32_t*, uint32_t*, uint32_t, const DevTex*);

void run_op(const std::string& dir, const char* inName, uint32_t inPlanes, const char* outName, uint32_t outWords,
            OpKernel kernel, const DevTex* aux = nullptr, uint32_t auxCount = 0)
{
    const std::vector<uint32_t> in = read_words(dir + "/" + inName);
    if (in.empty() || in.size() % inPlanes != 0 || in.size() / inPlanes > 0x7fffffffu / 8u)
        fail(std::string(inName) + ": not a whole number of inputs");
    const uint32_t n = (uint32_t)(in.size() / inPlanes);
    if (aux)
        for (uint32_t i = 0; i < n; ++i)
            if (in[i] >= auxCount) fail(std::string(inName) + ": texture index beyond the table");
    uint32_t* din = to_device(in);
    uint32_t* dout = nullptr;
    std::vector<uint32_t> out((size_t)n * outWords);
    CHECK(hipMalloc(&dout, out.size() * 4));
    CHECK(hipMemset(dout, 0xff, out.size() * 4));
    kernel<<<(n + 255u) / 256u, 256, 0, 0>>>(din, dout, n, aux);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    write_words(dir + "/" + outName, out);
}

void run_stream(const std::string& dir)
{
    std::vector<uint32_t> in = read_words(dir + "/xorwow_stream.in");
    if (in.size() < 3 || in.size() % 2 != 1) fail("xorwow_stream.in: want n and pairs of seed words");
    const uint32_t draws = in[0], n = (uint32_t)(in.size() / 2);
    if (draws == 0 || draws > (1u << 22) || n > 64) fail("xorwow_stream.in: at most 2^22 draws of at most 64 seeds");
    in.erase(in.begin());
    uint32_t* din = to_device(in);
    uint32_t* dout = nullptr;
    std::vector<uint32_t> out(2 * (size_t)draws * n);
    CHECK(hipMalloc(&dout, out.size() * 4));
    CHECK(hipMemset(dout, 0xff, out.size() * 4));
    k_xorwow_stream<<<(n + 255u) / 256u, 256, 0, 0>>>(din, dout, n, draws);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    write_words(dir + "/xorwow_stream.out", out);
}

// tex2d.tab -> the device's table of descriptors (each texture's texels in one allocation)
const DevTex* load_textures(const std::string& dir, uint32_t& count)
{
    const std::vector<uint32_t> tab = read_words(dir + "/tex2d.tab");
    if (tab.empty() || tab[0] == 0 || tab[0] > 64 || tab.size() < 1 + 2 * (size_t)tab[0]) fail("tex2d.tab: bad header");
    count = tab[0];
    std::vector<DevTex> host(count);
    size_t at = 1 + 2 * (size_t)count;
    for (uint32_t t = 0; t < count; ++t) {
        const uint32_t w = tab[1 + 2 * t], h = tab[2 + 2 * t];
        if (w == 0 || h == 0 || w > 8192 || h > 8192) fail("tex2d.tab: bad texture size");
        const size_t words = 4 * (size_t)w * h;
        if (at + words > tab.size()) fail("tex2d.tab: texels missing");
        float4* d = nullptr;
        CHECK(hipMalloc(&d, words * 4));
        CHECK(hipMemcpy(d, tab.data() + at, words * 4, hipMemcpyHostToDevice));
        host[t] = DevTex{d, w, h, (float)w, (float)h};
        at += words;
    }
    if (at != tab.size()) fail("tex2d.tab: trailing words");
    DevTex* dev = nullptr;
    CHECK(hipMalloc(&dev, count * sizeof(DevTex)));
    CHECK(hipMemcpy(dev, host.data(), count * sizeof(DevTex), hipMemcpyHostToDevice));
    return dev;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 2) fail("usage: dev_functions DIR");
    const std::string dir = argv[1];
    run_op(dir, "sincos_pos.in", 1, "sincos_pos.out", 2, k_sincos_pos);
    run_op(dir, "acos.in", 1, "acos_.out", 1, k_acos);
    run_op(dir, "acos.in", 1, "acos_sel.out", 1, k_acos_sel);
    run_op(dir, "atan2.in", 2, "atan2_.out", 1, k_atan2);
    run_op(dir, "atan2.in", 2, "atan2_sel.out", 1, k_atan2_sel);
    run_op(dir, "log.in", 1, "log_.out", 1, k_log);
    run_op(dir, "exp.in", 1, "exp_.out", 1, k_exp);
    run_op(dir, "pow.in", 2, "pow_.out", 1, k_pow);
    run_op(dir, "f2i.in", 1, "f2i_x86.out", 1, k_f2i);
    run_op(dir, "tonemap.in", 4, "tonemap_pixel.out", 1, k_tonemap);
    uint32_t texCount = 0;
    const DevTex* textures = load_textures(dir, texCount);
    run_op(dir, "tex2d.in", 3, "tex2d.out", 3, k_tex2d, textures, texCount);
    run_op(dir, "xorwow_init.in", 2, "xorwow_init.out", 6, k_xorwow_init);
    run_op(dir, "xorwow_skip.in", 3, "xorwow_skip.out", 6, k_xorwow_skip);
    run_stream(dir);
    printf("dev_functions: 15 operations done\n");
    return 0;
}
