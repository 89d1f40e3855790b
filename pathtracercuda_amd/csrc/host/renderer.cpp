// Pathtracer: host owner of one device context (reference src/pathtracer/Pathtracer.cpp:30-339).
// Host side keeps the reference's responsibilities: BVH build + validation on setScene, texture
// decode on loadTexture, the accumulated-frame counter and the two normalisations of
// getHDRImageData / getImageData.  Device work goes through the C ABI of include/pt_hip.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_internal.h"
#include "pathtracer_amd.hpp"

namespace ptamd {
thread_local bool g_throwOnError = false;
}

void Pathtracer::check(int rc, const char* what) const
{
    if (rc == PT_OK) return;
    char buf[1024];
    const char* detail = m_group ? pt_group_last_error(m_group) : (m_ctx ? pt_last_error(m_ctx) : "");
    snprintf(buf, sizeof(buf), "HIP error = %d at %s '%s'", rc, what, detail);
    if (ptamd::g_throwOnError) throw ptamd::Error(rc, buf);
    // reference behaviour (Pathtracer.cpp:17-28): report and terminate
    fprintf(stderr, "%s\n", buf);
    exit(EXIT_FAILURE);
}

// a refusal of this class's own, before any device call
void Pathtracer::refuse(int rc, const char* msg) const
{
    if (ptamd::g_throwOnError) throw ptamd::Error(rc, msg);
    fprintf(stderr, "%s\n", msg);
    exit(EXIT_FAILURE);
}

Pathtracer::Pathtracer(uint32_t width, uint32_t height, unsigned int openglPixelBuffer)
    : Pathtracer(width, height, 0, 0u, 1u)
{
    if (openglPixelBuffer != 0) {
        const char* msg = "OpenGL pixel-buffer interop is not supported (headless renderer)";
        if (ptamd::g_throwOnError) throw ptamd::Error(PT_ERR_ARG, msg);
        fprintf(stderr, "%s\n", msg);
        exit(EXIT_FAILURE);
    }
}

Pathtracer::Pathtracer(uint32_t width, uint32_t height, int device, uint32_t rowOffset, uint32_t rowStride)
    : Pathtracer(width, height, Tile{device, 1u, rowOffset, rowStride})
{
}

Pathtracer::Pathtracer(uint32_t width, uint32_t height, const Tile& tile)
    : m_width(width), m_height(height)
{
    check(pt_create_banded(tile.device, width, height, tile.bandRows, tile.bandOffset, tile.bandStride, &m_ctx),
          "pt_create_banded");
    allocHostBuffers();
}

Pathtracer::Pathtracer(uint32_t width, uint32_t height, const std::vector<int>& devices, uint32_t bandRows)
    : m_width(width), m_height(height)
{
    // the reference hard-codes device 0 (Pathtracer.cpp:40); here every listed device renders a
    // share of the row bands and RCCL assembles the image on devices[0]
    check(pt_group_create((int)devices.size(), devices.data(), width, height, bandRows, &m_group), "pt_group_create");
    m_ctx = pt_group_context(m_group, 0);
    allocHostBuffers();
}

void Pathtracer::allocHostBuffers()
{
    const size_t npix = (size_t)localRows() * m_width;
    m_cpuAccumBuffer.resize(npix * 4);
    m_cpuResultBuffer.resize(npix * 4);
}

Pathtracer::~Pathtracer()
{
    if (m_group) pt_group_destroy(m_group);
    else pt_destroy(m_ctx);
}

uint32_t Pathtracer::localRows() const { return m_group ? m_height : pt_local_rows(m_ctx); }

void Pathtracer::setScene(size_t count, const CpuHittable* hittables)
{
    if (count == 0) {
        printf("Setting an empty scene is not allowed!\n");
        return;
    }
    m_bvh = BVH();
    m_bvh.build(count, hittables, 4);
    if (!m_bvh.validate()) check(PT_ERR_STATE, "BVH::validate");   // reference: assert(bvh.validate())
    const auto& nodes = m_bvh.getNodes();
    const auto& elems = m_bvh.getElements();
    std::vector<pt_bvh_node> dn(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) dn[i] = ptamd::toDeviceNode(nodes[i]);
    std::vector<pt_hittable> dp(elems.size());
    for (size_t i = 0; i < elems.size(); ++i) dp[i] = elems[i].getGpuHittable();
    if (m_group)
        check(pt_group_set_scene(m_group, dn.data(), (uint32_t)dn.size(), dp.data(), (uint32_t)dp.size()), "pt_group_set_scene");
    else
        check(pt_set_scene(m_ctx, dn.data(), (uint32_t)dn.size(), dp.data(), (uint32_t)dp.size()), "pt_set_scene");
    m_nodeCount = (uint32_t)dn.size();
    m_hittableCount = (uint32_t)dp.size();
    m_denoised = false;
    m_despiked = false;
    m_upsampled = false;
    rememberScene(count, hittables);
    m_motionRows.clear();
    m_motionPrev.clear();
}

// The objects in the caller's order, and where BVH::build put each: an element is matched to the first object
// not yet taken whose device record is the same words (objects that are word for word the same are interchangeable
// to the tracer; taking them in order keeps the match deterministic).
void Pathtracer::rememberScene(size_t count, const CpuHittable* hittables)
{
    std::vector<CpuHittable> objects(hittables, hittables + count);   // (hittables may point into m_sceneObjects)
    const auto key = [](const CpuHittable& h) {
        const pt_hittable g = h.getGpuHittable();
        return std::string((const char*)&g, sizeof(g));
    };
    std::map<std::string, std::vector<uint32_t>> byWords;
    for (size_t k = count; k-- > 0;) byWords[key(objects[k])].push_back((uint32_t)k);   // popped from the back: in order
    const auto& elems = m_bvh.getElements();
    m_objectToPrim.assign(count, 0xffffffffu);
    for (size_t p = 0; p < elems.size(); ++p) {
        auto it = byWords.find(key(elems[p]));
        if (it == byWords.end() || it->second.empty()) check(PT_ERR_STATE, "setScene: a BVH element matches no object");
        m_objectToPrim[it->second.back()] = (uint32_t)p;
        it->second.pop_back();
    }
    m_sceneObjects.swap(objects);
}

void Pathtracer::setSceneMoved(size_t count, const CpuHittable* hittables, const uint32_t* previousObject)
{
    if (m_group) check(PT_ERR_STATE, "setSceneMoved: not available on a device group");
    if (count == 0) {
        printf("Setting an empty scene is not allowed!\n");
        return;
    }
    if (m_sceneObjects.empty()) {       // nothing to move from
        setScene(count, hittables);
        return;
    }
    const size_t prevCount = m_sceneObjects.size();
    char msg[200];
    if (!previousObject && count != prevCount) {
        snprintf(msg, sizeof(msg), "setSceneMoved: the scene has %zu objects and the previous one %zu "
                 "(give previousObject when the counts differ)", count, prevCount);
        refuse(PT_ERR_ARG, msg);
    }
    for (size_t k = 0; previousObject && k < count; ++k)
        if (previousObject[k] != 0xffffffffu && previousObject[k] >= prevCount) {
            snprintf(msg, sizeof(msg), "setSceneMoved: previousObject[%zu] = %u is neither 0xffffffff nor below the "
                     "previous scene's %zu objects", k, previousObject[k], prevCount);
            refuse(PT_ERR_ARG, msg);
        }
    // per object: the map and the primitive it was in the previous BVH
    std::vector<float> objRows(12 * count, 0.0f);
    std::vector<uint32_t> objPrev(count, 0xffffffffu);
    for (size_t k = 0; k < count; ++k) {
        const uint32_t j = previousObject ? previousObject[k] : (uint32_t)k;
        if (j == 0xffffffffu) continue;
        if (ptamd::motionRows(m_sceneObjects[j].invTransformRows(), hittables[k].invTransformRows(), &objRows[12 * k]))
            objPrev[k] = m_objectToPrim[j];
    }
    BVH bvh;
    bvh.build(count, hittables, 4);
    if (!bvh.validate()) check(PT_ERR_STATE, "BVH::validate");
    const BVH before = m_bvh;
    const std::vector<CpuHittable> objectsBefore = m_sceneObjects;
    const std::vector<uint32_t> permBefore = m_objectToPrim;
    m_bvh = bvh;
    rememberScene(count, hittables);
    const auto& nodes = m_bvh.getNodes();
    const auto& elems = m_bvh.getElements();
    std::vector<pt_bvh_node> dn(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) dn[i] = ptamd::toDeviceNode(nodes[i]);
    std::vector<pt_hittable> dp(elems.size());
    for (size_t i = 0; i < elems.size(); ++i) dp[i] = elems[i].getGpuHittable();
    std::vector<float> rows(12 * elems.size());
    std::vector<uint32_t> prev(elems.size());
    for (size_t k = 0; k < count; ++k) {
        const uint32_t p = m_objectToPrim[k];
        memcpy(&rows[12 * (size_t)p], &objRows[12 * k], 12 * sizeof(float));
        prev[p] = objPrev[k];
    }
    const int rc = pt_set_scene_moved(m_ctx, dn.data(), (uint32_t)dn.size(), dp.data(), (uint32_t)dp.size(), rows.data(),
                                      prev.data());
    if (rc != PT_OK) {                  // refused: the device keeps the previous scene, and so does this class
        m_bvh = before;
        m_sceneObjects = objectsBefore;
        m_objectToPrim = permBefore;
        check(rc, "pt_set_scene_moved");
    }
    m_motionRows.swap(rows);
    m_motionPrev.swap(prev);
    m_nodeCount = (uint32_t)dn.size();
    m_hittableCount = (uint32_t)dp.size();
    m_denoised = false;
    m_despiked = false;
    m_upsampled = false;
}

void Pathtracer::moveObjects(size_t count, const uint32_t* object, const CpuHittable* hittables)
{
    if (m_group) check(PT_ERR_STATE, "moveObjects: not available on a device group");
    if (m_sceneObjects.empty()) refuse(PT_ERR_STATE, "moveObjects: no scene is set");
    if (count == 0 || !object || !hittables) refuse(PT_ERR_ARG, "moveObjects: count is 0 or an array is null");
    const size_t n = m_sceneObjects.size();
    char msg[200];
    std::vector<char> seen(n, 0);
    for (size_t k = 0; k < count; ++k) {
        if (object[k] >= n) {
            snprintf(msg, sizeof(msg), "moveObjects: object[%zu] = %u is not below the scene's %zu objects", k, object[k], n);
            refuse(PT_ERR_ARG, msg);
        }
        if (seen[object[k]]) {
            snprintf(msg, sizeof(msg), "moveObjects: object %u is given twice", object[k]);
            refuse(PT_ERR_ARG, msg);
        }
        seen[object[k]] = 1;
    }
    std::vector<uint32_t> index(count), prev(count);
    std::vector<pt_hittable> dp(count);
    std::vector<float> boxes(6 * count), rows(12 * count);
    for (size_t k = 0; k < count; ++k) {
        index[k] = m_objectToPrim[object[k]];
        dp[k] = hittables[k].getGpuHittable();
        const AABB& b = hittables[k].getAABB();
        for (int a = 0; a < 3; ++a) {
            boxes[6 * k + a] = b.m_min[a];
            boxes[6 * k + 3 + a] = b.m_max[a];
        }
        const bool ok = ptamd::motionRows(m_sceneObjects[object[k]].invTransformRows(), hittables[k].invTransformRows(), &rows[12 * k]);
        prev[k] = ok ? index[k] : 0xffffffffu;
    }
    if (!pt_holds_primitive_boxes(m_ctx)) {          // the first move, or the first since a scene or texture change
        const auto& elems = m_bvh.getElements();
        std::vector<float> all(6 * elems.size());
        for (size_t i = 0; i < elems.size(); ++i) {
            const AABB& b = elems[i].getAABB();
            for (int a = 0; a < 3; ++a) {
                all[6 * i + a] = b.m_min[a];
                all[6 * i + 3 + a] = b.m_max[a];
            }
        }
        check(pt_set_primitive_boxes(m_ctx, all.data()), "pt_set_primitive_boxes");
    }
    check(pt_move_primitives(m_ctx, (uint32_t)count, index.data(), dp.data(), boxes.data(), rows.data(), prev.data()),
          "pt_move_primitives");
    // accepted: this class mirrors what the device holds now
    m_bvh.refit(count, index.data(), hittables);
    for (size_t k = 0; k < count; ++k) m_sceneObjects[object[k]] = hittables[k];
    const size_t np = m_bvh.getElements().size();
    m_motionRows.assign(12 * np, 0.0f);
    m_motionPrev.resize(np);
    for (size_t p = 0; p < np; ++p) {
        m_motionRows[12 * p] = m_motionRows[12 * p + 5] = m_motionRows[12 * p + 10] = 1.0f;
        m_motionPrev[p] = (uint32_t)p;
    }
    for (size_t k = 0; k < count; ++k) {
        memcpy(&m_motionRows[12 * (size_t)index[k]], &rows[12 * k], 12 * sizeof(float));
        m_motionPrev[index[k]] = prev[k];
    }
    m_denoised = false;
    m_despiked = false;
    m_upsampled = false;
}

void Pathtracer::rebuildScene()
{
    if (m_group) check(PT_ERR_STATE, "rebuildScene: not available on a device group");
    if (m_sceneObjects.empty()) refuse(PT_ERR_STATE, "rebuildScene: no scene is set");
    const std::vector<CpuHittable> objects = m_sceneObjects;
    setSceneMoved(objects.size(), objects.data());
}

float Pathtracer::refitTiming()
{
    if (m_group) check(PT_ERR_STATE, "refitTiming: not available on a device group");
    float ms[3] = {};
    check(pt_read_refit_timing(m_ctx, ms), "pt_read_refit_timing");
    return ms[0];
}

bool Pathtracer::holdsMotion() const { return !m_group && pt_holds_motion(m_ctx) != 0; }

void Pathtracer::render(const Camera& camera, uint32_t spp, bool ignoreHistory)
{
    renderChunks(camera, spp, 1, ignoreHistory);
}

void Pathtracer::renderChunks(const Camera& camera, uint32_t spp, uint32_t chunks, bool ignoreHistory)
{
    // after renderAdaptive the pixels hold different numbers of calls: one frame counter cannot
    // normalise a buffer that goes on accumulating (ignoreHistory starts a uniform buffer again)
    if (adaptive() && !ignoreHistory)
        check(PT_ERR_STATE, "render: the buffer holds an adaptive render; continue it with renderAdaptive(reset = false) "
                            "or start over with ignoreHistory");
    m_timing = 0.0f;
    const pt_camera cam = camera.toDevice();
    float ms = 0.0f;
    if (m_group) check(pt_group_render(m_group, &cam, spp, chunks, ignoreHistory ? 1 : 0, &ms), "pt_group_render");
    else check(pt_render(m_ctx, &cam, spp, chunks, ignoreHistory ? 1 : 0, &ms), "pt_render");
    // the flags move once the call has succeeded: a refused render changes nothing, and one that launched
    // nothing (spp or chunks 0) leaves an adaptive buffer adaptive
    m_adaptive = adaptive();
    m_denoised = false;
    m_despiked = false;
    m_upsampled = false;
    if (ignoreHistory) m_accumulatedFrames = 0;
    m_timing = ms;
    m_accumulatedFrames += chunks;
}

// m_adaptive says that this class made an adaptive render; the device context says whether its per-pixel
// counts still describe the buffer (a pt_render on the context, past this class, ends that too)
bool Pathtracer::adaptive() const { return m_adaptive && !m_group && pt_holds_adaptive(m_ctx) != 0; }

Pathtracer::AdaptiveResult Pathtracer::renderAdaptive(const Camera& camera, uint32_t spp, uint32_t minCalls, uint32_t maxCalls,
                                                      float tolerance, float floor, bool reset)
{
    if (m_group) check(PT_ERR_STATE, "renderAdaptive: not available on a device group");
    if (!reset && !adaptive()) check(PT_ERR_STATE, "renderAdaptive: reset = false needs a previous adaptive render");
    m_timing = 0.0f;
    const pt_camera cam = camera.toDevice();
    const pt_adaptive_params ap = {spp, minCalls, maxCalls, tolerance, floor, reset ? 1 : 0};
    pt_adaptive_result res = {};
    check(pt_render_adaptive(m_ctx, &cam, &ap, &res), "pt_render_adaptive");
    m_timing = res.gpu_ms;
    m_adaptive = true;
    m_denoised = false;
    m_despiked = false;
    m_upsampled = false;
    m_accumulatedFrames = 0;          // the per-pixel counts describe the buffer now
    return AdaptiveResult{res.rounds, res.samples, res.gpu_ms};
}

void Pathtracer::renderFeatures(const Camera& camera)
{
    if (m_group) check(PT_ERR_STATE, "renderFeatures: not available on a device group");
    const pt_camera cam = camera.toDevice();
    check(pt_render_features(m_ctx, &cam), "pt_render_features");
    m_despiked = false;               // a despiked image was of the planes held before
}

const float* Pathtracer::featurePlane(uint32_t plane)
{
    if (m_group) check(PT_ERR_STATE, "featurePlane: not available on a device group");
    m_featureBuffer.resize((size_t)localRows() * m_width * 4);
    check(pt_read_features(m_ctx, plane, m_featureBuffer.data()), "pt_read_features");
    return m_featureBuffer.data();
}

float Pathtracer::denoise(const DenoiseOptions& o)
{
    if (m_group) check(PT_ERR_STATE, "denoise: not available on a device group");
    pt_denoise_params p = {o.iterations, o.sigmaColor, o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    if (!(o.sigmaColor > 0.0f)) {
        // automatic: a factor times the median luminance of the kept pixels' (demodulated) colour
        const size_t npix = (size_t)localRows() * m_width;
        const bool was = m_denoised;   // the statistic is of the image to be filtered; a refusal below changes nothing
        m_denoised = false;
        const float* c = nullptr;
        try {
            c = getHDRImageData();
        } catch (...) {
            m_denoised = was;
            throw;
        }
        m_denoised = was;
        std::vector<float> a(npix * 4), n(npix * 4), q(npix * 4), lum;
        check(pt_read_features(m_ctx, 0, a.data()), "pt_read_features");
        check(pt_read_features(m_ctx, 1, n.data()), "pt_read_features");
        check(pt_read_features(m_ctx, 2, q.data()), "pt_read_features");
        lum.reserve(npix);
        for (size_t i = 0; i < npix; ++i) {
            uint32_t fl;
            memcpy(&fl, &q[4 * i + 3], 4);
            bool keep = (fl & PT_FEATURE_HIT) && !(fl & PT_FEATURE_EMISSIVE);
            float v[3];
            for (int k = 0; k < 3; ++k) {
                keep = keep && std::isfinite(c[4 * i + k]) && std::isfinite(n[4 * i + k]) && std::isfinite(q[4 * i + k]);
                const float d = (o.flags & PT_DENOISE_DEMODULATE) ? fmaxf(a[4 * i + k], 1.0f / 64.0f) : 1.0f;
                v[k] = c[4 * i + k] / d;
            }
            if (keep) lum.push_back((0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2]);
        }
        p.sigma_color = 1.0f;
        if (!lum.empty()) {
            std::sort(lum.begin(), lum.end());
            const size_t h = lum.size() / 2;
            const float med = (lum.size() & 1) ? lum[h] : 0.5f * (lum[h - 1] + lum[h]);
            if (med > 0.0f && std::isfinite(med)) p.sigma_color = PT_DENOISE_DEFAULT_SIGMA_FACTOR * med;
        }
    }
    if (despiked()) check(pt_denoise_despiked(m_ctx, &p), "pt_denoise_despiked");
    else check(pt_denoise(m_ctx, m_accumulatedFrames, &p), "pt_denoise");
    m_denoised = true;
    m_upsampled = false;
    return p.sigma_color;
}

void Pathtracer::despike(const DespikeOptions& o)
{
    if (m_group) check(PT_ERR_STATE, "despike: not available on a device group");
    // minNeighbors 0: the default, raised to rank and lowered to what the window has (Python's rule)
    const uint32_t side = 2u * o.radius + 1u, taps = side * side - 1u;
    const uint32_t minNeighbors = o.minNeighbors ? o.minNeighbors
                                                 : std::min(std::max((uint32_t)PT_DESPIKE_DEFAULT_MIN_NEIGHBORS, o.rank), taps);
    const pt_despike_params p = {o.radius, o.rank, o.factor, o.floor, minNeighbors, o.sigmaPlane, o.normalCosMin, o.flags, o.staging};
    check(pt_despike(m_ctx, m_accumulatedFrames, &p), "pt_despike");
    m_despiked = true;
    m_upsampled = false;
    m_denoised = false;               // a denoised image was of the image before the clamp
}

// m_despiked says that this class made a despiked image and has ended it nowhere; the device context says whether
// it is still held (a call on the context, past this class, ends it too)
bool Pathtracer::despiked() const { return m_despiked && !m_group && pt_holds_despiked(m_ctx) != 0; }

void Pathtracer::upsample(Pathtracer& lo, const UpsampleOptions& o)
{
    if (m_group || lo.m_group) check(PT_ERR_STATE, "upsample: not available on a device group");
    uint32_t source = o.source;
    if (source == kUpsampleAuto)
        source = lo.m_denoised ? PT_UPSAMPLE_DENOISED : (lo.despiked() ? PT_UPSAMPLE_DESPIKED : PT_UPSAMPLE_ACCUM);
    const pt_upsample_params p = {o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    check(pt_upsample(m_ctx, lo.m_ctx, source, lo.m_accumulatedFrames, &p), "pt_upsample");
    m_upsampled = true;
}

void Pathtracer::upsample(Pathtracer& lo, Pathtracer& planes, const UpsampleOptions& o)
{
    if (m_group || lo.m_group || planes.m_group) check(PT_ERR_STATE, "upsample: not available on a device group");
    uint32_t source = o.source;
    if (source == kUpsampleAuto)
        source = lo.m_denoised ? PT_UPSAMPLE_DENOISED : (lo.despiked() ? PT_UPSAMPLE_DESPIKED : PT_UPSAMPLE_ACCUM);
    const pt_upsample_params p = {o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    const uint32_t factor = planes.m_width / m_width;         // (anything but exactly 2..4 times this frame is refused below)
    check(pt_upsample_resolve(m_ctx, planes.m_ctx, lo.m_ctx, source, lo.m_accumulatedFrames, factor, &p), "pt_upsample_resolve");
    m_upsampled = true;
}

// (as despiked(): the class's flag and the context's fact)
bool Pathtracer::upsampled() const { return m_upsampled && !m_group && pt_holds_upsampled(m_ctx) != 0; }

void Pathtracer::upsampleCounts(uint32_t counts[2])
{
    if (m_group) check(PT_ERR_STATE, "upsampleCounts: not available on a device group");
    check(pt_read_upsample_counts(m_ctx, counts), "pt_read_upsample_counts");
}

uint32_t Pathtracer::despikeCount()
{
    if (m_group) check(PT_ERR_STATE, "despikeCount: not available on a device group");
    uint32_t n = 0;
    check(pt_read_despike_count(m_ctx, &n), "pt_read_despike_count");
    return n;
}

bool Pathtracer::temporal(const TemporalOptions& o, bool reset)
{
    if (m_group) check(PT_ERR_STATE, "temporal: not available on a device group");
    const pt_temporal_params p = {o.alphaMin, o.maxHistory, o.sigmaPlane, o.normalCosMin, o.flags};
    int used = 0;
    check(pt_temporal(m_ctx, m_accumulatedFrames, &p, reset ? 1 : 0, &used), "pt_temporal");
    return used != 0;
}

float* Pathtracer::getTemporalHDRImageData()
{
    if (m_group) check(PT_ERR_STATE, "getTemporalHDRImageData: not available on a device group");
    m_temporalBuffer.resize((size_t)localRows() * m_width * 4);
    check(pt_read_temporal(m_ctx, m_temporalBuffer.data()), "pt_read_temporal");
    return m_temporalBuffer.data();
}

bool Pathtracer::temporalMoments(const TemporalOptions& o, uint32_t minTemporal, bool reset)
{
    if (m_group) check(PT_ERR_STATE, "temporalMoments: not available on a device group");
    const pt_temporal_params p = {o.alphaMin, o.maxHistory, o.sigmaPlane, o.normalCosMin, o.flags};
    const pt_variance_params v = {minTemporal};
    int used = 0;
    check(pt_temporal_moments(m_ctx, m_accumulatedFrames, &p, &v, reset ? 1 : 0, &used), "pt_temporal_moments");
    return used != 0;
}

const float* Pathtracer::temporalVariance()
{
    if (m_group) check(PT_ERR_STATE, "temporalVariance: not available on a device group");
    m_varianceBuffer.resize((size_t)localRows() * m_width);
    check(pt_read_temporal_variance(m_ctx, m_varianceBuffer.data()), "pt_read_temporal_variance");
    return m_varianceBuffer.data();
}

void Pathtracer::denoiseVariance(const VarianceDenoiseOptions& o)
{
    if (m_group) check(PT_ERR_STATE, "denoiseVariance: not available on a device group");
    const pt_vdenoise_params p = {o.iterations, o.sigmaL, o.varianceFloor, o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    check(pt_denoise_variance(m_ctx, &p), "pt_denoise_variance");
    m_denoised = true;
    m_upsampled = false;
}

void Pathtracer::denoiseVariance(const VarianceDenoiseOptions& o, uint32_t feedbackLevel)
{
    if (m_group) check(PT_ERR_STATE, "denoiseVariance: not available on a device group");
    const pt_vdenoise_params p = {o.iterations, o.sigmaL, o.varianceFloor, o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    const pt_vfeedback_params f = {feedbackLevel};
    check(pt_denoise_variance_feedback(m_ctx, &p, &f), "pt_denoise_variance_feedback");
    m_denoised = true;
    m_upsampled = false;
}

void Pathtracer::denoiseAdaptive(const AdaptiveVarianceOptions& a, const VarianceDenoiseOptions& o)
{
    if (m_group) check(PT_ERR_STATE, "denoiseAdaptive: not available on a device group");
    const pt_adaptive_variance_params v = {a.minBatches, a.sigmaPlane, a.normalCosMin, a.flags};
    const pt_vdenoise_params p = {o.iterations, o.sigmaL, o.varianceFloor, o.sigmaPlane, o.normalPowerLog2, o.flags, o.staging};
    check(pt_denoise_adaptive(m_ctx, &v, &p), "pt_denoise_adaptive");
    m_denoised = true;
    m_upsampled = false;
}

const float* Pathtracer::adaptiveVariance()
{
    if (m_group) check(PT_ERR_STATE, "adaptiveVariance: not available on a device group");
    m_varianceBuffer.resize((size_t)localRows() * m_width);
    check(pt_read_adaptive_variance(m_ctx, m_varianceBuffer.data()), "pt_read_adaptive_variance");
    return m_varianceBuffer.data();
}

const float* Pathtracer::temporalHistory(uint32_t plane)
{
    if (m_group) check(PT_ERR_STATE, "temporalHistory: not available on a device group");
    m_historyBuffer.resize((size_t)localRows() * m_width * 4);
    check(pt_read_temporal_history(m_ctx, plane, m_historyBuffer.data()), "pt_read_temporal_history");
    return m_historyBuffer.data();
}

float Pathtracer::getTiming() const { return m_timing; }

uint32_t Pathtracer::loadTexture(const char* path)
{
    if (m_textureCount >= PT_MAX_TEXTURES) return 0;
    std::vector<float> rgba;
    uint32_t w = 0, h = 0;
    std::string err;
    if (!ptamd::loadImageRGBA32F(path, rgba, w, h, err)) return 0;     // failure -> null handle
    uint64_t hash = 1469598103934665603ull;                            // FNV-1a over the pixel words
    for (const float v : rgba) {
        uint32_t u;
        memcpy(&u, &v, 4);
        for (int k = 0; k < 4; ++k) hash = (hash ^ ((u >> (8 * k)) & 0xffu)) * 1099511628211ull;
    }
    if (m_reuseTextures) {
        // the sky's own handle first (only that one leaves the sky as it is), then the latest load with these pixels
        const auto same = [&](size_t i) {
            return m_textureKeys[i].width == w && m_textureKeys[i].height == h && m_textureKeys[i].hash == hash;
        };
        if (m_skyboxTextureHandle >= 1 && m_skyboxTextureHandle <= m_textureKeys.size() && same(m_skyboxTextureHandle - 1))
            return m_skyboxTextureHandle;
        for (size_t i = m_textureKeys.size(); i-- > 0;)
            if (same(i)) return (uint32_t)i + 1;
    }
    if (m_group) check(pt_group_set_texture(m_group, m_textureCount + 1, rgba.data(), w, h), "pt_group_set_texture");
    else check(pt_set_texture(m_ctx, m_textureCount + 1, rgba.data(), w, h), "pt_set_texture");
    ++m_textureCount;
    m_textureKeys.push_back({w, h, hash});
    m_despiked = false;
    m_upsampled = false;
    return m_textureCount;
}

void Pathtracer::setSkyboxTextureHandle(uint32_t handle)
{
    if (handle != m_skyboxTextureHandle) m_despiked = m_upsampled = false;     // the image's colours are of the old sky
    m_skyboxTextureHandle = handle;
    if (m_group) check(pt_group_set_skybox(m_group, handle), "pt_group_set_skybox");
    else check(pt_set_skybox(m_ctx, handle), "pt_set_skybox");
}

float* Pathtracer::getHDRImageData()
{
    if (upsampled()) {
        check(pt_read_upsampled(m_ctx, m_cpuAccumBuffer.data()), "pt_read_upsampled");
        return m_cpuAccumBuffer.data();
    }
    if (m_denoised) {
        check(pt_read_denoised(m_ctx, m_cpuAccumBuffer.data()), "pt_read_denoised");
        return m_cpuAccumBuffer.data();
    }
    if (despiked()) {
        check(pt_read_despiked(m_ctx, m_cpuAccumBuffer.data()), "pt_read_despiked");
        return m_cpuAccumBuffer.data();
    }
    if (adaptive()) {                 // every pixel over its own number of calls
        check(pt_read_adaptive_hdr(m_ctx, m_cpuAccumBuffer.data()), "pt_read_adaptive_hdr");
        return m_cpuAccumBuffer.data();
    }
    if (m_group) {
        check(pt_group_gather(m_group, &m_gatherMs), "pt_group_gather");
        check(pt_group_read_accum(m_group, m_cpuAccumBuffer.data()), "pt_group_read_accum");
    } else {
        check(pt_read_accum(m_ctx, m_cpuAccumBuffer.data()), "pt_read_accum");
    }
    const float inv = 1.0f / fmaxf((float)m_accumulatedFrames, 1.0f);   // Pathtracer.cpp:307
    for (float& v : m_cpuAccumBuffer) v *= inv;
    return m_cpuAccumBuffer.data();
}

char* Pathtracer::getImageData()
{
    if (upsampled()) {
        check(pt_tonemap_upsampled(m_ctx, (uint8_t*)m_cpuResultBuffer.data()), "pt_tonemap_upsampled");
        return m_cpuResultBuffer.data();
    }
    if (m_denoised) {
        check(pt_tonemap_denoised(m_ctx, (uint8_t*)m_cpuResultBuffer.data()), "pt_tonemap_denoised");
        return m_cpuResultBuffer.data();
    }
    if (despiked()) {
        check(pt_tonemap_despiked(m_ctx, (uint8_t*)m_cpuResultBuffer.data()), "pt_tonemap_despiked");
        return m_cpuResultBuffer.data();
    }
    if (adaptive()) {
        check(pt_tonemap_adaptive(m_ctx, (uint8_t*)m_cpuResultBuffer.data()), "pt_tonemap_adaptive");
        return m_cpuResultBuffer.data();
    }
    if (m_group) check(pt_group_tonemap(m_group, m_accumulatedFrames, (uint8_t*)m_cpuResultBuffer.data()), "pt_group_tonemap");
    else check(pt_tonemap(m_ctx, m_accumulatedFrames, (uint8_t*)m_cpuResultBuffer.data()), "pt_tonemap");
    return m_cpuResultBuffer.data();
}
