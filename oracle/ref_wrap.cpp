// C ABI over the reference's own source, compiled for the host.  TEST INFRASTRUCTURE ONLY.
//
// Nothing of the reference is restated here.  Its files are reached through #include alone, at build
// time, from the tree named by the REF make variable (oracle/Makefile, target `ref`): the three
// kernels below, and Hittable.cpp and BVH.cpp as translation units of their own.  The CUDA
// vocabulary they need comes from oracle/ref_shim/.  cuRAND, the texture sampler and CUDA's libm
// are not in that tree and come from liboracle.so (see ref_shim/cuda_runtime.h).
//
// Driven by oracle/pyref.py; compared with the oracle, the host layer and the HIP kernel by
// tests/test_ref_source.py and tests/test_gpu_ref_source.py.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "cuda_runtime.h"
#include "curand_kernel.h"

#include "kernels/initRandState.cu"
#include "kernels/tonemap.cu"
#include "kernels/trace.cu"

#define REF_EXPORT extern "C" __attribute__((visibility("default")))

// The layouts the oracle, the host layer and the HIP kernel share (or_sizeof in pt_oracle.c).
static_assert(sizeof(float4) == 16 && alignof(float4) == 16, "float4 is 16-byte aligned in CUDA");
static_assert(sizeof(Material) == 40, "Material");
static_assert(sizeof(Hittable) == 96, "Hittable");
static_assert(sizeof(BVHNode) == 32, "BVHNode");
static_assert(sizeof(Camera) == 92, "Camera");
static_assert(sizeof(AABB) == 24, "AABB");
static_assert(sizeof(curandState) == 24, "XORWOW state");
static_assert(sizeof(uchar4) == 4, "uchar4");
static_assert(sizeof(ptref_texture) == 16, "texture record");
#ifndef __CUDA_ARCH__
#error "Material::sample must see __CUDA_ARCH__ (Material.inl:26)"
#endif

namespace {

struct RefScene {
    std::vector<CpuHittable> input;          // constructor products, file order
    BVH bvh;
    std::vector<Hittable> world;             // getGpuHittable() of the BVH's elements, BVH order
    std::vector<BVHNode> nodes;
    std::vector<ptref_texture> textures;
    std::vector<cudaTextureObject_t> handles;
    uint32_t skybox = 0;
};

struct KernelScope {                          // device code runs between ctor and dtor
    KernelScope() { ptref_shim::in_kernel = true; }
    ~KernelScope() { ptref_shim::in_kernel = false; }
};

// The reference launches every kernel with 8x8 threads on ceil(w/8) x ceil(h/8) blocks
// (Pathtracer.cpp:52-53,176-177,326-327).
template <class F> void launch(uint32_t width, uint32_t height, F &&thread_body)
{
    KernelScope scope;
    blockDim = dim3(8, 8, 1);
    const dim3 blocks((width + 7) / 8, (height + 7) / 8, 1);
    for (unsigned by = 0; by < blocks.y; ++by)
        for (unsigned bx = 0; bx < blocks.x; ++bx)
            for (unsigned ty = 0; ty < blockDim.y; ++ty)
                for (unsigned tx = 0; tx < blockDim.x; ++tx) {
                    blockIdx = { bx, by, 0 };
                    threadIdx = { tx, ty, 0 };
                    thread_body();
                }
    blockIdx = { 0, 0, 0 };
    threadIdx = { 0, 0, 0 };
    blockDim = dim3(1, 1, 1);
}

vec3 v3(const float *p) { return vec3(p[0], p[1], p[2]); }

void put_aabb(const AABB &b, float *out)
{
    out[0] = b.m_min.x; out[1] = b.m_min.y; out[2] = b.m_min.z;
    out[3] = b.m_max.x; out[4] = b.m_max.y; out[5] = b.m_max.z;
}

void put_hittable(const Hittable &h, uint8_t *out)
{
    // rows (48) + material (40) + type (4); the four tail bytes are padding in the reference and
    // zero in the other layers
    std::memset(out, 0, sizeof(Hittable));
    std::memcpy(out, static_cast<const void *>(&h), 92);
}

Camera load_camera(const void *bytes)
{
    Camera c(vec3(0.0f), vec3(0.0f, 0.0f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 1.0f, 1.0f);
    std::memcpy(static_cast<void *>(&c), bytes, sizeof(Camera));
    return c;
}

}  // namespace

REF_EXPORT uint32_t ref_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(Material);
    case 1: return sizeof(Hittable);
    case 2: return sizeof(CpuHittable);
    case 3: return sizeof(BVHNode);
    case 4: return sizeof(Camera);
    case 5: return sizeof(curandState);
    case 6: return sizeof(ptref_texture);
    default: return 0;
    }
}

// Scene from plain arrays (rotation in radians): Material and CpuHittable constructors, then
// BVH::build(count, elements, 4) and getGpuHittable() as Pathtracer::setScene does.
REF_EXPORT void *ref_scene_create(uint32_t count, const uint32_t *types, const float *positions, const float *rotations,
                                  const float *scales, const uint32_t *materialTypes, const float *baseColors,
                                  const float *emissives, const float *roughness, const float *metalness,
                                  const uint32_t *textureHandles)
{
    if (count == 0) return nullptr;
    RefScene *s = new RefScene();
    s->input.reserve(count);
    for (uint32_t i = 0; i < count; ++i) {
        Material m(static_cast<MaterialType>(materialTypes[i]), v3(baseColors + 3 * i), v3(emissives + 3 * i),
                   roughness[i], metalness[i], textureHandles[i]);
        s->input.push_back(CpuHittable(static_cast<HittableType>(types[i]), v3(positions + 3 * i), v3(rotations + 3 * i),
                                       v3(scales + 3 * i), m));
    }
    s->bvh.build(count, s->input.data(), 4);
    s->nodes = s->bvh.getNodes();
    for (const CpuHittable &e : s->bvh.getElements()) s->world.push_back(e.getGpuHittable());
    return s;
}

REF_EXPORT void ref_scene_free(void *scene) { delete static_cast<RefScene *>(scene); }

REF_EXPORT uint32_t ref_scene_node_count(const void *scene)
{
    return static_cast<uint32_t>(static_cast<const RefScene *>(scene)->nodes.size());
}

REF_EXPORT int ref_scene_validate(void *scene) { return static_cast<RefScene *>(scene)->bvh.validate() ? 1 : 0; }

REF_EXPORT uint32_t ref_scene_depth(const void *scene) { return static_cast<const RefScene *>(scene)->bvh.getDepth(); }

// Constructor products in file order: 96-byte hittables and (min, max) boxes.
REF_EXPORT void ref_scene_objects(const void *scene, uint8_t *hittables, float *aabbs)
{
    const RefScene *s = static_cast<const RefScene *>(scene);
    for (size_t i = 0; i < s->input.size(); ++i) {
        put_hittable(s->input[i].getGpuHittable(), hittables + 96 * i);
        put_aabb(s->input[i].getAABB(), aabbs + 6 * i);
    }
}

// The built BVH: 32-byte nodes, and the hittables and boxes in the order the build left them.
REF_EXPORT void ref_scene_bvh(const void *scene, uint8_t *nodes, uint8_t *hittables, float *aabbs)
{
    const RefScene *s = static_cast<const RefScene *>(scene);
    std::memcpy(nodes, s->nodes.data(), s->nodes.size() * sizeof(BVHNode));
    const std::vector<CpuHittable> &e = s->bvh.getElements();
    for (size_t i = 0; i < e.size(); ++i) {
        put_hittable(s->world[i], hittables + 96 * i);
        put_aabb(e[i].getAABB(), aabbs + 6 * i);
    }
}

// textures[handle - 1]; the texel arrays stay owned by the caller and must outlive the scene's use.
REF_EXPORT void ref_scene_set_textures(void *scene, uint32_t count, const ptref_texture *textures, uint32_t skyboxHandle)
{
    RefScene *s = static_cast<RefScene *>(scene);
    s->textures.assign(textures, textures + count);
    s->handles.clear();
    for (const ptref_texture &t : s->textures) s->handles.push_back(static_cast<cudaTextureObject_t>(reinterpret_cast<uintptr_t>(&t)));
    s->skybox = skyboxHandle;
}

REF_EXPORT void ref_camera_make(const float *position, const float *lookat, const float *up, float fovy, float aspect,
                                void *out)
{
    Camera c(v3(position), v3(lookat), v3(up), fovy, aspect);
    std::memcpy(out, &c, sizeof(Camera));
}

REF_EXPORT void ref_camera_rotate(void *camera, float pitch, float yaw, float roll)
{
    Camera c = load_camera(camera);
    c.rotate(pitch, yaw, roll);
    std::memcpy(camera, &c, sizeof(Camera));
}

REF_EXPORT void ref_camera_translate(void *camera, float x, float y, float z)
{
    Camera c = load_camera(camera);
    c.translate(x, y, z);
    std::memcpy(camera, &c, sizeof(Camera));
}

REF_EXPORT void ref_init_rand_state(uint32_t width, uint32_t height, void *states)
{
    curandState *st = static_cast<curandState *>(states);
    launch(width, height, [&] { initRandState(static_cast<int>(width), static_cast<int>(height), st); });
}

// One Pathtracer::render call (Pathtracer.cpp:162-227) without the display path: traceKernel for
// every thread of every block.  accum is width * height float4, states width * height XORWOW states.
REF_EXPORT void ref_render(void *scene, const void *camera, uint32_t width, uint32_t height, float *accum, void *states,
                           uint32_t spp, int ignoreHistory, uint32_t accumulatedFrames)
{
    RefScene *s = static_cast<RefScene *>(scene);
    const Camera cam = load_camera(camera);
    float4 *acc = reinterpret_cast<float4 *>(accum);
    curandState *st = static_cast<curandState *>(states);
    launch(width, height, [&] {
        traceKernel(acc, ignoreHistory != 0, accumulatedFrames, width, height, spp, static_cast<uint32_t>(s->world.size()),
                    s->world.data(), static_cast<uint32_t>(s->nodes.size()), s->nodes.data(), st, cam, s->skybox,
                    s->handles.data());
    });
}

REF_EXPORT void ref_tonemap(const float *accum, uint32_t width, uint32_t height, uint32_t frames, uint8_t *out)
{
    float4 *acc = reinterpret_cast<float4 *>(const_cast<float *>(accum));
    launch(width, height, [&] { tonemap(reinterpret_cast<uchar4 *>(out), acc, width, height, frames); });
}
