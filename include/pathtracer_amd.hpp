// pathtracer_amd.hpp -- C++ drop-in API of the MI355X path tracer (libpt_host.so).
//
// Mirrors the public host surface of DoerriesT/PathtracerCUDA so its callers (SceneLoader.cpp,
// main.cpp) build unchanged against this library:
//   vec3 ops                 src/pathtracer/vec3.h:7-57
//   Camera                   src/pathtracer/Camera.h:4-23
//   Material / MaterialType  src/pathtracer/Material.h:9-32
//   CpuHittable / HittableType src/pathtracer/Hittable.h:9-56
//   BVHNode / BVH            src/pathtracer/BVH.h:6-31
//   Pathtracer               src/pathtracer/Pathtracer.h:12-68
//   Params                   src/Params.h:4-13
//   loadScene                src/SceneLoader.h:9, SceneLoader.cpp:124-348
// Differences (all additive): a Pathtracer can own a row-band tile of a larger image or span
// several GPUs of the process (RCCL gather), a device index can be chosen, and renderChunks()
// runs several render() calls in one launch.
// All host arithmetic follows the reference operation for operation (built with
// -ffp-contract=off) so BVHs, transforms and cameras are bit-identical to the reference's.
#pragma once

#include <cstddef>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_hip.h"

// ------------------------------------------------------------------------------------------------
// vec3 (vec3.h / vec3.inl semantics: v / s == (1 / s) * v, min uses <, max uses >=)
// ------------------------------------------------------------------------------------------------
#define PT_PI (3.14159265358979323846f)

struct vec3 {
    union {
        struct { float x, y, z; };
        struct { float r, g, b; };
        float e[3];
    };
    vec3() : e{0.0f, 0.0f, 0.0f} {}
    vec3(float e0, float e1, float e2) : e{e0, e1, e2} {}
    vec3(float s) : e{s, s, s} {}
    vec3 operator-() const { return vec3(-e[0], -e[1], -e[2]); }
    float operator[](int i) const { return e[i]; }
    float& operator[](int i) { return e[i]; }
    vec3& operator+=(const vec3& v) { e[0] += v.e[0]; e[1] += v.e[1]; e[2] += v.e[2]; return *this; }
    vec3& operator*=(float t) { e[0] *= t; e[1] *= t; e[2] *= t; return *this; }
    vec3& operator*=(const vec3& t) { e[0] *= t.x; e[1] *= t.y; e[2] *= t.z; return *this; }
    vec3& operator/=(float t) { return *this *= 1 / t; }
};

inline vec3 operator+(const vec3& u, const vec3& v) { return vec3(u.e[0] + v.e[0], u.e[1] + v.e[1], u.e[2] + v.e[2]); }
inline vec3 operator+(const vec3& u, float v) { return vec3(u.e[0] + v, u.e[1] + v, u.e[2] + v); }
inline vec3 operator+(float u, const vec3& v) { return v + u; }
inline vec3 operator-(const vec3& u, const vec3& v) { return vec3(u.e[0] - v.e[0], u.e[1] - v.e[1], u.e[2] - v.e[2]); }
inline vec3 operator-(const vec3& u, float v) { return vec3(u.e[0] - v, u.e[1] - v, u.e[2] - v); }
inline vec3 operator-(float u, const vec3& v) { return -v + u; }
inline vec3 operator*(const vec3& u, const vec3& v) { return vec3(u.e[0] * v.e[0], u.e[1] * v.e[1], u.e[2] * v.e[2]); }
inline vec3 operator*(float t, const vec3& v) { return vec3(t * v.e[0], t * v.e[1], t * v.e[2]); }
inline vec3 operator*(const vec3& v, float t) { return t * v; }
inline vec3 operator/(const vec3& v, const vec3& t) { return vec3(1.0f / t.x, 1.0f / t.y, 1.0f / t.z) * v; }
inline vec3 operator/(const vec3& v, float t) { return (1.0f / t) * v; }
inline vec3 operator/(float v, const vec3& t) { return vec3(1.0f / t.x, 1.0f / t.y, 1.0f / t.z) * v; }
inline bool operator==(const vec3& u, const vec3& v) { return u.x == v.x && u.y == v.y && u.z == v.z; }
inline float dot(const vec3& u, const vec3& v) { return u.e[0] * v.e[0] + u.e[1] * v.e[1] + u.e[2] * v.e[2]; }
inline vec3 cross(const vec3& u, const vec3& v)
{
    return vec3(u.e[1] * v.e[2] - u.e[2] * v.e[1], u.e[2] * v.e[0] - u.e[0] * v.e[2], u.e[0] * v.e[1] - u.e[1] * v.e[0]);
}
float length(const vec3& v);
inline vec3 min(const vec3& a, const vec3& b)
{
    return vec3(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.z < b.z ? a.z : b.z);
}
inline vec3 max(const vec3& a, const vec3& b)
{
    return vec3(a.x >= b.x ? a.x : b.x, a.y >= b.y ? a.y : b.y, a.z >= b.z ? a.z : b.z);
}
inline vec3 normalize(const vec3& v) { return v / length(v); }
vec3 rotateAroundVector(const vec3& v, const vec3& axis, float cosAngle, float sinAngle);

// ------------------------------------------------------------------------------------------------
// Camera (Camera.h / Camera.inl); fovy in radians
// ------------------------------------------------------------------------------------------------
class Camera {
public:
    Camera(const vec3& position, const vec3& lookat, const vec3& up, float fovy, float aspectRatio);
    void rotate(float pitch, float yaw, float roll);
    void translate(float x, float y, float z);
    void update();
    pt_camera toDevice() const;

    float m_tanHalfFovy;
    float m_aspectRatio;
    vec3 m_origin;
    vec3 m_lowerLeftCorner;
    vec3 m_horizontal;
    vec3 m_vertical;
    vec3 m_right;
    vec3 m_up;
    vec3 m_backward;
};

// ------------------------------------------------------------------------------------------------
// Material, shapes
// ------------------------------------------------------------------------------------------------
enum class MaterialType : uint32_t { LAMBERT, GGX, LAMBERT_GGX };
enum class HittableType : uint32_t { SPHERE, CYLINDER, DISK, CONE, PARABOLOID, QUAD, CUBE };

class Material {
public:
    Material(MaterialType type = MaterialType::LAMBERT, const vec3& baseColor = vec3(1.0f), const vec3& emissive = vec3(0.0f),
             float roughness = 0.5f, float metalness = 0.0f, uint32_t textureIndex = 0);

    vec3 m_baseColor;
    float m_roughness;
    vec3 m_emissive;
    float m_metalness;
    uint32_t m_textureIndex;
    MaterialType m_materialType;
};

struct AABB {
    vec3 m_min;
    vec3 m_max;
};

// Scene object with the data needed to build the BVH (Hittable.h:40-56); rotation in radians.
class CpuHittable {
public:
    CpuHittable();
    CpuHittable(HittableType type, const vec3& position, const vec3& rotation, const vec3& scale, const Material& material);
    const AABB& getAABB() const { return m_aabb; }
    pt_hittable getGpuHittable() const;
    HittableType type() const { return m_type; }
    const float* invTransformRows() const { return &m_invTransformRows[0][0]; }
    const Material& material() const { return m_material; }
    // what the constructor was given (rotation in radians); the default object: the origin, no rotation, scale 1
    const vec3& position() const { return m_position; }
    const vec3& rotation() const { return m_rotation; }
    const vec3& scale() const { return m_scale; }

private:
    vec3 m_position = vec3(0.0f), m_rotation = vec3(0.0f), m_scale = vec3(1.0f);
    float m_invTransformRows[3][4];
    Material m_material;
    AABB m_aabb;
    HittableType m_type;
};

// ------------------------------------------------------------------------------------------------
// BVH (BVH.h): binned SAH, 8 bins x 3 axes, depth-first layout, left child = node + 1
// ------------------------------------------------------------------------------------------------
struct BVHNode {
    AABB m_aabb;
    uint32_t m_offset;
    uint32_t m_primitiveCountAxis;
};

class BVH {
public:
    void build(size_t elementCount, const CpuHittable* elements, uint32_t maxLeafElements);
    const std::vector<BVHNode>& getNodes() const { return m_nodes; }
    const std::vector<CpuHittable>& getElements() const { return m_elements; }
    uint32_t getDepth(uint32_t node = 0) const;
    bool validate();
    // Elements elementIndex[k] replaced by elements[k] and every node's box refitted (rule 10 of pt_hip.h,
    // ptamd::refitBoxes): the topology stays.  What Pathtracer::moveObjects does to its mirror of the device's tree.
    void refit(size_t count, const uint32_t* elementIndex, const CpuHittable* elements);

private:
    uint32_t m_maxLeafElements = 1;
    std::vector<BVHNode> m_nodes;
    std::vector<CpuHittable> m_elements;
    uint32_t buildInto(std::vector<BVHNode>& out, size_t begin, size_t end);
    std::atomic<int>* m_spareThreads = nullptr;   // worker-thread budget during build()
    bool validateRecursive(uint32_t node, std::vector<char>& reached);
};

// ------------------------------------------------------------------------------------------------
// Pathtracer (Pathtracer.h:12-68)
// ------------------------------------------------------------------------------------------------
class Pathtracer {
public:
    // openglPixelBuffer is accepted for source compatibility; GL interop is not supported (must be 0).
    explicit Pathtracer(uint32_t width, uint32_t height, unsigned int openglPixelBuffer = 0);
    // Row tile of a width x height image on `device`: rows y = rowOffset + k * rowStride.
    Pathtracer(uint32_t width, uint32_t height, int device, uint32_t rowOffset, uint32_t rowStride);
    // Band tile on `device`: the bands of bandRows rows b = bandOffset + k * bandStride
    // (pt_create_banded); bandRows = 1 is the row tile above.
    struct Tile {
        int device;
        uint32_t bandRows, bandOffset, bandStride;
    };
    Pathtracer(uint32_t width, uint32_t height, const Tile& tile);
    // The whole image on several GPUs of this process (the CLI's -gpus N): device i renders the row
    // bands i, i + N, ... and getHDRImageData / getImageData return the full image, gathered on
    // devices[0] over RCCL (pt_group_*).  Bit-identical to a single-device render.
    Pathtracer(uint32_t width, uint32_t height, const std::vector<int>& devices, uint32_t bandRows = 8);
    Pathtracer(const Pathtracer&) = delete;
    Pathtracer(const Pathtracer&&) = delete;
    Pathtracer& operator=(const Pathtracer&) = delete;
    Pathtracer& operator=(const Pathtracer&&) = delete;
    ~Pathtracer();

    void setScene(size_t count, const CpuHittable* hittables);
    // setScene for a scene whose objects moved since the last setScene / setSceneMoved, keeping the temporal history
    // (pt_set_scene_moved, rule 7 of pt_hip.h).  previousObject[k] = the index object k had in the last scene's
    // array, or 0xffffffff for an object that was not there; null: object k was object k, and the counts must then
    // match.  The per-object maps come from the two scenes' transforms (ptamd::motionRows); the per-primitive table,
    // with its indices in the last scene's BVH order, is kept (motionRows, motionPrevIndex: one entry per primitive
    // of the new BVH).  An object whose map is not finite takes no history.  Without an earlier scene the call is
    // setScene.  One move per temporal step: a second move before the next temporal() ends the history.  Objects
    // that are word for word the same are told apart by their order in the array.  Single device only.
    void setSceneMoved(size_t count, const CpuHittable* hittables, const uint32_t* previousObject = nullptr);
    // Move objects without a rebuild (pt_move_primitives, rule 10 of pt_hip.h): object[k], an index into the last
    // scene's array, becomes hittables[k].  An upload of the moved objects' records and a refit of the existing tree on
    // the device (only the upload scales with what moved: the refit, here and on the device, and the motion table run over
    // the whole scene); the temporal history is kept exactly as setSceneMoved keeps it (the motion rows come from the two
    // transforms; one move per temporal step), and motionRows / motionPrevIndex answer as after setSceneMoved.  The
    // tree is afterwards no longer the one BVH::build would make for the new poses: renders equal the oracle walking
    // bvh(), which this class keeps equal to the device's tree; rebuildScene() returns to the build's tree.  Refused,
    // with nothing of this class or the device changed: a device group, no scene, count 0, a null array, an index
    // out of range or given twice, whatever pt_move_primitives refuses.
    void moveObjects(size_t count, const uint32_t* object, const CpuHittable* hittables);
    // setSceneMoved of the current objects onto themselves: a fresh SAH tree, the history kept.  For when a refitted
    // tree has grown slow.
    void rebuildScene();
    const std::vector<CpuHittable>& sceneObjects() const { return m_sceneObjects; }
    float refitTiming();                             // pt_read_refit_timing of the last moveObjects, ms
    bool holdsMotion() const;                        // a motion table is held for the next temporal step
    const std::vector<float>& motionRows() const { return m_motionRows; }
    const std::vector<uint32_t>& motionPrevIndex() const { return m_motionPrev; }
    void render(const Camera& camera, uint32_t spp, bool ignoreHistory);
    // `chunks` successive render(camera, spp, ...) calls in one launch (first one honours
    // ignoreHistory); bit-identical to the loop.  Timing covers the whole launch.
    void renderChunks(const Camera& camera, uint32_t spp, uint32_t chunks, bool ignoreHistory);
    // Adaptive sampling (pt_render_adaptive, pt_hip.h): calls of spp samples per pixel until the
    // standard error of the pixel's per-call luminance is below tolerance x (|mean| + floor), at least
    // minCalls and at most maxCalls calls.  Afterwards getHDRImageData / getImageData divide every
    // pixel by its own number of calls, and render(..., ignoreHistory = false) is an error until a
    // render with ignoreHistory starts a uniform buffer again.  Single device only.
    struct AdaptiveResult {
        uint32_t rounds;      // trace launches
        uint64_t samples;     // camera paths traced
        float gpuMs;
    };
    AdaptiveResult renderAdaptive(const Camera& camera, uint32_t spp, uint32_t minCalls, uint32_t maxCalls, float tolerance,
                                  float floor = 0.01f, bool reset = true);
    // The buffer holds an adaptive render: from renderAdaptive until the next launch that writes the
    // accumulation, through this class or through the device layer (pt_holds_adaptive).  A scene, texture or
    // sky change does not end it: the image calls go on dividing every pixel by its own number of calls.
    bool adaptive() const;
    // First-hit feature buffers and the edge-avoiding a-trous denoiser (pt_render_features, pt_denoise,
    // pt_hip.h).  renderFeatures traces each pixel's first-sample ray and keeps three float4 planes (albedo +
    // primitive, normal + distance, position + flags); featurePlane returns one (borrowed, rows x width x 4).
    // denoise filters the image guided by them: afterwards getHDRImageData / getImageData return the
    // denoised image until the next render or scene change; the accumulation itself is not touched, so
    // rendering continues as if the pass had not run.  sigmaColor <= 0: automatic (the factor of
    // PT_DENOISE_DEFAULT_SIGMA_FACTOR times the median luminance of the kept pixels).  Single device only.
    struct DenoiseOptions {
        uint32_t iterations = PT_DENOISE_DEFAULT_ITERATIONS;
        float sigmaColor = 0.0f;
        float sigmaPlane = PT_DENOISE_DEFAULT_SIGMA_PLANE;
        uint32_t normalPowerLog2 = PT_DENOISE_DEFAULT_NORMAL_POWER_LOG2;
        uint32_t flags = PT_DENOISE_DEFAULT_FLAGS;
        uint32_t staging = 0;
    };
    void renderFeatures(const Camera& camera);
    const float* featurePlane(uint32_t plane);
    float denoise(const DenoiseOptions& options);    // returns the sigma_color used
    float denoise() { return denoise(DenoiseOptions()); }
    bool denoised() const { return m_denoised; }     // the image calls return the denoised image
    // Despike, the same-surface firefly clamp (pt_despike, rule 6 of pt_hip.h), after render and renderFeatures: a
    // pixel whose luminance stands above `factor` times the `rank`-th largest of its same-surface neighbours within
    // `radius`, plus `floor`, is scaled down to that limit; every other pixel keeps its words.  While the despiked
    // image is held (until the next render, renderFeatures, scene, texture or sky change) getHDRImageData /
    // getImageData return it and denoise() filters it (pt_denoise_despiked); the accumulation is not touched.
    // despikeCount: the pixels the last despike clamped.  Single device only.
    struct DespikeOptions {
        uint32_t radius = PT_DESPIKE_DEFAULT_RADIUS;
        uint32_t rank = PT_DESPIKE_DEFAULT_RANK;
        float factor = PT_DESPIKE_DEFAULT_FACTOR;
        float floor = PT_DESPIKE_DEFAULT_FLOOR;
        uint32_t minNeighbors = 0;   // 0: PT_DESPIKE_DEFAULT_MIN_NEIGHBORS, raised to rank and lowered to the window's taps
        float sigmaPlane = PT_DESPIKE_DEFAULT_SIGMA_PLANE;
        float normalCosMin = PT_DESPIKE_DEFAULT_NORMAL_COS_MIN;
        uint32_t flags = PT_DESPIKE_DEFAULT_FLAGS;
        uint32_t staging = 0;
    };
    void despike(const DespikeOptions& options);
    void despike() { despike(DespikeOptions()); }
    uint32_t despikeCount();
    bool despiked() const;                           // a despiked image made through this class is still held
    // Guided upsampling (pt_upsample, rule 8 of pt_hip.h): this Pathtracer reconstructs its frame from the image of
    // `lo`, a Pathtracer of the same scene and camera at a lower resolution on the same device.  Both need
    // renderFeatures(camera); this one needs no render.  source: one of PT_UPSAMPLE_*, or kUpsampleAuto = what lo's
    // image calls return (its denoised image, else its despiked image, else its accumulation over its frames or
    // per-pixel counts).  While the upsampled image is held (until the next render, scene, texture or sky change or
    // filter call on this Pathtracer) getHDRImageData / getImageData return it.  Nothing of `lo` changes.
    // upsampleCounts: the pixels that needed the wider ring, and those that took the nearest low pixel.  Single device only.
    static constexpr uint32_t kUpsampleAuto = 0xffffffffu;
    struct UpsampleOptions {
        uint32_t source = kUpsampleAuto;
        float sigmaPlane = PT_UPSAMPLE_DEFAULT_SIGMA_PLANE;
        uint32_t normalPowerLog2 = PT_UPSAMPLE_DEFAULT_NORMAL_POWER_LOG2;
        uint32_t flags = PT_UPSAMPLE_DEFAULT_FLAGS;
        uint32_t staging = 0;
    };
    void upsample(Pathtracer& lo, const UpsampleOptions& options);
    void upsample(Pathtracer& lo) { upsample(lo, UpsampleOptions()); }
    // The same onto the planes of `planes`, a Pathtracer of the same scene and camera at exactly 2, 3 or 4 times this
    // one's width and height that has had renderFeatures(camera): every pixel is the mean of the results at its S x S
    // first-hit samples, so silhouettes are antialiased (pt_upsample_resolve, rule 9 of pt_hip.h).  This Pathtracer then
    // needs neither features nor a render; nothing of `lo` or `planes` changes.
    void upsample(Pathtracer& lo, Pathtracer& planes, const UpsampleOptions& options);
    void upsample(Pathtracer& lo, Pathtracer& planes) { upsample(lo, planes, UpsampleOptions()); }
    void upsampleCounts(uint32_t counts[2]);
    bool upsampled() const;                          // an upsampled image made through this class is still held
    // Temporal reprojection (pt_temporal, pt_hip.h): per frame render(camera, spp, true), renderFeatures(camera),
    // temporal().  The result of the previous temporal() is reprojected into this frame's camera, rejected
    // where it is no longer the same surface, and this frame blended in.  Returns whether a previous history
    // was used (none after reset, a scene load, a texture or another sky).  getTemporalHDRImageData returns the
    // image (borrowed, rows x width x 4, w = the history length); getHDRImageData / getImageData and the
    // accumulation are not changed.  Single device only.
    struct TemporalOptions {
        float alphaMin = PT_TEMPORAL_DEFAULT_ALPHA_MIN;
        uint32_t maxHistory = PT_TEMPORAL_DEFAULT_MAX_HISTORY;
        float sigmaPlane = PT_TEMPORAL_DEFAULT_SIGMA_PLANE;
        float normalCosMin = PT_TEMPORAL_DEFAULT_NORMAL_COS_MIN;
        uint32_t flags = PT_TEMPORAL_DEFAULT_FLAGS;
    };
    bool temporal(const TemporalOptions& options, bool reset = false);
    bool temporal() { return temporal(TemporalOptions()); }
    float* getTemporalHDRImageData();
    // The temporal step with luminance moments and the per-pixel variance estimated from them
    // (pt_temporal_moments, pt_hip.h): temporal()'s image word for word; temporalVariance returns the variance
    // (borrowed, rows x width floats, -1 where the pixel is not a finite hit).  denoiseVariance filters the
    // temporal image with a colour weight that follows that variance (pt_denoise_variance); its result is a
    // denoised image: the image calls return it as they do denoise()'s.  A history left by temporal() has no
    // moments: temporalMoments then starts anew and returns false.  Single device only.
    struct VarianceDenoiseOptions {
        uint32_t iterations = PT_VDENOISE_DEFAULT_ITERATIONS;
        float sigmaL = PT_VDENOISE_DEFAULT_SIGMA_L;
        float varianceFloor = PT_VDENOISE_DEFAULT_VARIANCE_FLOOR;
        float sigmaPlane = PT_VDENOISE_DEFAULT_SIGMA_PLANE;
        uint32_t normalPowerLog2 = PT_VDENOISE_DEFAULT_NORMAL_POWER_LOG2;
        uint32_t flags = PT_VDENOISE_DEFAULT_FLAGS;
        uint32_t staging = 0;
    };
    bool temporalMoments(const TemporalOptions& options, uint32_t minTemporal = PT_VARIANCE_DEFAULT_MIN_TEMPORAL,
                         bool reset = false);
    bool temporalMoments() { return temporalMoments(TemporalOptions()); }
    const float* temporalVariance();
    void denoiseVariance(const VarianceDenoiseOptions& options);
    void denoiseVariance() { denoiseVariance(VarianceDenoiseOptions()); }
    // The same filter and the same result, and the output of iteration feedbackLevel - 1 (1..iterations) becomes
    // the colour of the held history, which the next temporalMoments reprojects (pt_denoise_variance_feedback).
    // temporalHistory: plane 0..3 of the held history (borrowed, rows x width float4; plane 3 only while the
    // history has moments).
    void denoiseVariance(const VarianceDenoiseOptions& options, uint32_t feedbackLevel);
    const float* temporalHistory(uint32_t plane);
    // The same filter after renderAdaptive and renderFeatures, its variance made from the adaptive render's own
    // per-pixel moments (pt_denoise_adaptive, rule 5 of pt_hip.h): a pixel with fewer than minBatches calls takes
    // the larger of its own batch-means estimate and the spread of its 7 x 7 same-surface window.  The result is a
    // denoised image, as denoiseVariance's; the DEMODULATE bits of the two option sets must agree.
    // adaptiveVariance: that variance (borrowed, rows x width floats, -1 where the rule gives none), until a render
    // writes the accumulation or renderFeatures runs.  Single device only.
    struct AdaptiveVarianceOptions {
        uint32_t minBatches = PT_AVARIANCE_DEFAULT_MIN_BATCHES;
        float sigmaPlane = PT_AVARIANCE_DEFAULT_SIGMA_PLANE;
        float normalCosMin = PT_AVARIANCE_DEFAULT_NORMAL_COS_MIN;
        uint32_t flags = PT_AVARIANCE_DEFAULT_FLAGS;
    };
    void denoiseAdaptive(const AdaptiveVarianceOptions& variance, const VarianceDenoiseOptions& options);
    void denoiseAdaptive()
    {
        VarianceDenoiseOptions options;
        options.sigmaL = PT_ADENOISE_DEFAULT_SIGMA_L;      // this source's sweep chose another sigma_l than the temporal one's
        denoiseAdaptive(AdaptiveVarianceOptions(), options);
    }
    const float* adaptiveVariance();
    float getTiming() const;
    uint32_t loadTexture(const char* path);
    // While set, loadTexture returns the handle of an already loaded texture with the same size and pixels and
    // uploads nothing (loadSceneMoved sets it: a texture upload ends the temporal history).
    void reuseTextures(bool on) { m_reuseTextures = on; }
    void setSkyboxTextureHandle(uint32_t handle);
    float* getHDRImageData();
    char* getImageData();

    // additions
    uint32_t width() const { return m_width; }
    uint32_t height() const { return m_height; }
    uint32_t localRows() const;     // rows of the image data this object returns
    uint32_t accumulatedFrames() const { return m_accumulatedFrames; }
    pt_context* context() const { return m_ctx; }    // device context (devices[0]'s for a group)
    pt_group* group() const { return m_group; }      // null unless multi-device
    int deviceCount() const { return m_group ? pt_group_size(m_group) : 1; }
    float lastGatherMs() const { return m_gatherMs; }
    const BVH& bvh() const { return m_bvh; }

private:
    uint32_t m_width;
    uint32_t m_height;
    uint32_t m_hittableCount = 0;
    uint32_t m_nodeCount = 0;
    float m_timing = 0.0f;
    uint32_t m_accumulatedFrames = 0;
    uint32_t m_textureCount = 0;
    uint32_t m_skyboxTextureHandle = 0;
    std::vector<float> m_cpuAccumBuffer;
    std::vector<char> m_cpuResultBuffer;
    pt_context* m_ctx = nullptr;
    pt_group* m_group = nullptr;
    float m_gatherMs = 0.0f;
    bool m_adaptive = false;
    bool m_denoised = false;
    bool m_despiked = false;           // this class made a despiked image and nothing through it has ended it
    bool m_upsampled = false;          // this class made an upsampled image and nothing through it has ended it
    std::vector<float> m_featureBuffer;
    std::vector<float> m_temporalBuffer;
    std::vector<float> m_varianceBuffer;
    std::vector<float> m_historyBuffer;
    BVH m_bvh;
    std::vector<CpuHittable> m_sceneObjects;     // the last scene's objects, in the caller's order
    std::vector<uint32_t> m_objectToPrim;        // their indices in m_bvh's element order
    std::vector<float> m_motionRows;             // the last setSceneMoved's table, 12 floats per primitive
    std::vector<uint32_t> m_motionPrev;
    struct TextureKey {
        uint32_t width, height;
        uint64_t hash;
    };
    std::vector<TextureKey> m_textureKeys;       // index = handle - 1
    bool m_reuseTextures = false;
    void rememberScene(size_t count, const CpuHittable* hittables);
    void allocHostBuffers();
    void check(int rc, const char* what) const;
    void refuse(int rc, const char* msg) const;
};

// ------------------------------------------------------------------------------------------------
// CLI parameters and scene loading (Params.h, SceneLoader.h)
// ------------------------------------------------------------------------------------------------
struct Params {
    unsigned int m_width = 1024;
    unsigned int m_height = 1024;
    unsigned int m_spp = 1024;
    const char* m_inputFilepath = nullptr;
    const char* m_outputFilepath = nullptr;
    bool m_showWindow = false;
    bool m_enableControls = false;
    bool m_outputHdr = false;
    // additions
    unsigned int m_chunk = 8;        // samples per render() call of the headless loop (main.cpp:272)
    bool m_singleLaunch = true;      // run all chunks in one launch (bit-identical; CLI -call_loop: false)
    float m_adaptive = -1.0f;        // CLI -adaptive <tolerance>: >= 0 renders adaptively, m_spp is the budget
    unsigned int m_minSpp = 0;       // CLI -minspp: samples every pixel gets (0 = two calls)
    bool m_despike = false;          // CLI -despike: the firefly clamp at its defaults before the image is written
    unsigned int m_upsample = 0;     // CLI -upsample K: trace at ceil(w / K) x ceil(h / K) and reconstruct the frame (0 = off)
    unsigned int m_upsampleAa = 0;   // CLI -upsample_aa S: with -upsample, S x S first-hit samples per pixel (0 = one)
    unsigned int m_denoise = 0;      // CLI -denoise [N]: a-trous iterations applied before the image is written (0 = off)
    bool m_denoiseAdaptive = false;  // CLI -denoise_guide adaptive: the filter follows the adaptive render's own variance
};

Camera loadScene(Pathtracer& pathtracer, const Params& params);
// loadScene through setSceneMoved: the file's objects against the last scene's (previousObject as there, one entry
// per object of the file, or null).  A texture of the file whose pixels are already loaded keeps its handle, so an
// unchanged texture or sky ends nothing; a texture whose pixels changed is uploaded and ends the history as before.
Camera loadSceneMoved(Pathtracer& pathtracer, const Params& params, const uint32_t* previousObject = nullptr);

namespace ptamd {

// Scene description produced by the JSON loader without touching a GPU.
struct SceneDesc {
    std::vector<CpuHittable> objects;
    std::vector<std::string> texturePaths;   // index = handle - 1 of successfully loaded textures
    uint32_t skyboxHandle = 0;
    bool hasObjects = false;                 // "objects" array present (setScene is called)
    bool hasSkybox = false;                  // "skybox" string present
    vec3 cameraPosition = vec3(0.0f);
    vec3 cameraLookAt = vec3(0.0f, 0.0f, -1.0f);
    float cameraFovyDegrees = 60.0f;
};

// Parses a scene file (SceneLoader.cpp:124-348 semantics).  `textureLoader` is called for each
// distinct texture path in order of first use and returns the handle (0 = failure).
bool parseSceneFile(const std::string& path, SceneDesc& out, std::string& error,
                    uint32_t (*textureLoader)(void* user, const std::string& path), void* user);

float radians(float degree);   // SceneLoader.cpp:193-196

// The map of rule 7 (pt_hip.h) for one object from its two world->object transforms (3 x 4 row-major, [A | b]):
// T = [inverse(A_prev) A_cur | inverse(A_prev) (b_cur - b_prev)], in float64 from the float32 words, rounded once
// to float32 (the operation order is written out at pth_motion_table, pt_host.h).  False when a word of T is not
// finite.
bool motionRows(const float* prevInvRows, const float* curInvRows, float* out);

// Rule 10 of pt_hip.h on the host: the boxes of every node reachable from the root refitted in place from one box per
// primitive (primCount x 6 floats: min xyz, max xyz); offsets, counts and unreachable nodes keep their words.  False,
// with `error` set and nothing changed, when the nodes are not a tree over the primitives or a box is not finite or
// not ordered.
bool refitBoxes(pt_bvh_node* nodes, uint32_t nodeCount, const float* boxes, uint32_t primCount, std::string& error);

// Image I/O (stb_image / stb_image_write semantics for the formats the project uses).
bool isHdrFile(const std::string& path);
bool loadImageRGBA32F(const std::string& path, std::vector<float>& rgba, uint32_t& w, uint32_t& h, std::string& error);
bool writePNG(const std::string& path, uint32_t w, uint32_t h, const uint8_t* rgba, bool flipVertically);
bool writeHDR(const std::string& path, uint32_t w, uint32_t h, const float* rgba, bool flipVertically);

} // namespace ptamd
