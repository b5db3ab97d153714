// Cameras.h -- ARenderer plug-in seam + Camera, mirroring src/Scene/Cameras/{ARenderer.h,
// PathTracingRenderer.{h,cpp},Camera.{h,cpp}} on top of the libcloudtrace C ABI.
#pragma once

#include "Exr.h"
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <filesystem>
#include <sstream>

#include "NetworkFile.h"
#include "Scene.h"

namespace DeepestScatter
{
    // What the reference passes around as optix::Program camera / optix::Buffer frameResultBuffer.
    struct CameraProgram
    {
        float3 eye{}, U{}, V{}, W{};
        bool valid = false;
    };

    class ARenderer                                                              // ARenderer.h:6-16
    {
    public:
        ARenderer() = default;
        virtual ~ARenderer() = default;

        virtual CameraProgram* getCamera() = 0;
        virtual void init() = 0;
        virtual void render(float* frameResultBuffer /* device pointer, W*H*4 floats, or nullptr */) = 0;
    };

    class PathTracingRenderer : public ARenderer                                // PathTracingRenderer.h:8-31
    {
    public:
        explicit PathTracingRenderer(std::shared_ptr<Context> context) : context(std::move(context)) {}
        ~PathTracingRenderer() override = default;

        CameraProgram* getCamera() override { return &camera; }

        void init() override                                                     // PathTracingRenderer.cpp:14-19
        {
            // all scene items have published their variables by now (installApp order, installers.cpp:32-35)
            if (context->created()) return;   // the context of an earlier task of the same cloud: Sun::init has re-lit it
            CtScene& s = context->scene;
            s.density_host = context->density.data();
            s.mie_host = context->mie.data();
            s.chopped_mie_host = context->choppedMie.data();
            s.mie_count = (uint32_t)context->mie.size();
            s.estimator = estimator;
            context->create();
            context->density.clear();
            context->density.shrink_to_fit();
        }

        void render(float* frameResultBuffer) override                           // PathTracingRenderer.cpp:21-31
        {
            if (context->group) throw std::runtime_error("the two-launch loop (--unfused) renders on one GPU only");
            applyCamera();
            Context::check(ct_render_subframe(context->handle, subframeId, frameResultBuffer), context->handle, "ct_render_subframe");
        }

        // The fused form of Camera::render's loop (Camera.cpp:189-200) for subframes first .. first + count - 1; `enqueue`: the
        // batch need not be waited for.  A renderer with another source of frames overrides it.
        virtual void renderAccumulate(uint32_t first, uint32_t count, bool enqueue)
        {
            applyCamera();
            context->renderAccumulate(first, count, enqueue);
        }

        void publishCamera() { applyCamera(); }   // for a caller that renders on the handle itself (Camera's adaptive frame)

        uint32_t subframeId = 0;        // context["subframeId"], set by Camera::render (Camera.cpp:191-192)
        int estimator = CT_EST_MARCH;   // CT_EST_DELTA: Woodcock tracking instead of the reference's fixed-step march
        inline static const std::string NAME = "PT";

    protected:
        void applyCamera()              // the pose Camera::updatePosition left, published once
        {
            if (!camera.valid) return;
            context->setCamera(camera.eye.data(), camera.U.data(), camera.V.data(), camera.W.data());
            camera.valid = false;
        }

        std::shared_ptr<Context> context;
        CameraProgram camera;
    };

    // The reference's neural renderers are ARenderers too: the same Camera loop, the frame made by the scattering network
    // (ct_network_render_subframe / ct_network_render_accumulate) instead of the estimator.  It keeps the path tracer's scene
    // set-up (init) and output name; the network lives on the context's handle and goes before it.  params.transform may
    // carry CT_NET_ADD_SINGLE_SCATTER (--net-direct): both entry points then add the sun's single-scatter term to the frame.
    // With --gpus the context is a group: one network per shard (ct_group_network_create), every shard renders its own tiles
    // (ct_group_network_render_accumulate), and the group's merge, tonemap and convergence test apply as for the estimator.
    class NetworkRenderer : public PathTracingRenderer
    {
    public:
        NetworkRenderer(std::shared_ptr<Context> context, std::shared_ptr<const NetworkFile> file, const CtNetworkRender& params)
            : PathTracingRenderer(std::move(context)), file(std::move(file)), params(params) {}
        ~NetworkRenderer() override
        {
            if (network) ct_network_destroy(network);
            if (groupNetwork) ct_group_network_destroy(groupNetwork);
        }

        void init() override
        {
            PathTracingRenderer::init();
            if (network || groupNetwork) return;
            CtNetworkDesc d{ CT_ABI_VERSION, file->blocks, file->width, file->aux, file->headLayers, file->weights.data(), file->weights.size() };
            if (context->group) Context::checkGroup(ct_group_network_create(context->group, &d, &groupNetwork), context->group, "ct_group_network_create");
            else Context::check(ct_network_create(context->handle, &d, &network), context->handle, "ct_network_create");
        }

        void render(float* frameResultBuffer) override
        {
            if (context->group) throw std::runtime_error("the two-launch loop (--unfused) renders on one GPU only");
            applyCamera();
            Context::check(ct_network_render_subframe(context->handle, network, &params, subframeId, frameResultBuffer), context->handle,
                           "ct_network_render_subframe");
        }

        void renderAccumulate(uint32_t first, uint32_t count, bool /*enqueue: every band waits for its record count*/) override
        {
            applyCamera();
            if (context->group)
            {
                Context::checkGroup(ct_group_network_render_accumulate(context->group, groupNetwork, &params, first, count), context->group,
                                    "ct_group_network_render_accumulate");
                return;
            }
            Context::check(ct_network_render_accumulate(context->handle, network, &params, first, count), context->handle,
                           "ct_network_render_accumulate");
        }

    protected:
        std::shared_ptr<const NetworkFile> file;
        CtNetworkRender params;
        CtNetwork network = nullptr;
        CtGroupNetwork groupNetwork = nullptr;   // with --gpus: one network per shard, destroyed before the group
    };

    // --bake-in FILE / --bake-out FILE / --bake-half (include/cloudtrace.h, "bake files" and "half tables"), for both baked
    // renderers below.  in: the table comes from ct_bake_load instead of a bake run.  half: the frames are interpolated from the
    // ct_bake_half copy of the table.  out: the table that renders -- the half copy with --bake-half -- is saved by ct_bake_save.
    struct BakeFiles
    {
        std::string in, out;
        bool half = false;
    };

    // What the two renderers do alike with their table once it exists: the half copy, the file, and which of the two renders.
    // With --gpus the table is a CtGroupBake (ct_group_bake_*): built across the group's GPUs, complete on every shard; `bake` is
    // then shard 0's, owned by the group bake, which is what the accessors and --bake-out work on.
    class BakeHolder
    {
    public:
        ~BakeHolder()
        {
            if (halfCopy) ct_bake_destroy(halfCopy);
            if (groupBake) ct_group_bake_destroy(groupBake);   // (before the networks and the group)
            else if (bake) ct_bake_destroy(bake);              // (before the network and the handle)
        }
        // The handle the table's accessors report through: the context's, or shard 0's.
        static CtHandle handleOf(const Context& context)
        {
            CtHandle h = context.handle;
            if (context.group) Context::checkGroup(ct_group_handle(context.group, 0, &h), context.group, "ct_group_handle");
            return h;
        }
        void adoptShard(const Context& context)   // behind every call that makes the group bake
        {
            Context::checkGroup(ct_group_bake_shard(groupBake, 0, &bake), context.group, "ct_group_bake_shard");
        }
        bool load(const Context& context, const BakeFiles& files)   // true: the table came from --bake-in
        {
            if (files.in.empty()) return false;
            if (!context.group) return load(context.handle, files);
            Context::checkGroup(ct_group_bake_load(context.group, files.in.c_str(), &groupBake), context.group, "ct_group_bake_load");
            adoptShard(context);
            return true;
        }
        CtBake shown() const { return halfCopy ? halfCopy : bake; }
        bool isHalf(CtHandle handle) const
        {
            uint32_t format = CT_BAKE_F32;
            Context::check(ct_bake_format(bake, &format), handle, "ct_bake_format");
            return format == CT_BAKE_F16;
        }
        bool load(CtHandle handle, const BakeFiles& files)   // true: the table came from --bake-in
        {
            if (files.in.empty()) return false;
            Context::check(ct_bake_load(handle, files.in.c_str(), &bake), handle, "ct_bake_load");
            return true;
        }
        void finish(CtHandle handle, const BakeFiles& files, bool save)   // behind every bake, load, update and retrace
        {
            if (halfCopy) ct_bake_destroy(halfCopy);
            halfCopy = nullptr;
            if (files.half && !isHalf(handle)) Context::check(ct_bake_half(handle, bake, &halfCopy), handle, "ct_bake_half");
            if (save && !files.out.empty()) Context::check(ct_bake_save(shown(), files.out.c_str()), handle, "ct_bake_save");
        }
        bool current(CtHandle handle) const
        {
            CtBakeInfo info;
            Context::check(ct_bake_info(shown(), &info), handle, "ct_bake_info");
            if (!info.current && isHalf(handle))
                throw std::runtime_error("--bake-in: the file holds a half table made under another light, and a half bake is final; bake again");
            return info.current != 0;
        }
        // One subframe, or `count` accumulated ones, from the table: ct_baked_render_*, or with a depth (--net-trace-depth K) the hybrid
        // frames of ct_baked_render_hybrid_*; on a group every GPU renders its own tiles.
        void render(const Context& context, const CtNetworkRender& params, uint32_t depth, uint32_t subframeId, float* frameResultBuffer) const
        {
            if (depth) Context::check(ct_baked_render_hybrid_subframe(context.handle, shown(), &params, depth, subframeId, frameResultBuffer), context.handle,
                                      "ct_baked_render_hybrid_subframe");
            else Context::check(ct_baked_render_subframe(context.handle, shown(), &params, subframeId, frameResultBuffer), context.handle,
                                "ct_baked_render_subframe");
        }
        void renderAccumulate(const Context& context, const CtNetworkRender& params, uint32_t depth, uint32_t first, uint32_t count) const
        {
            if (context.group && depth)
                Context::checkGroup(ct_group_baked_render_hybrid_accumulate(context.group, groupBake, &params, depth, first, count), context.group,
                                    "ct_group_baked_render_hybrid_accumulate");
            else if (context.group)
                Context::checkGroup(ct_group_baked_render_accumulate(context.group, groupBake, &params, first, count), context.group,
                                    "ct_group_baked_render_accumulate");
            else if (depth)
                Context::check(ct_baked_render_hybrid_accumulate(context.handle, shown(), &params, depth, first, count), context.handle,
                               "ct_baked_render_hybrid_accumulate");
            else
                Context::check(ct_baked_render_accumulate(context.handle, shown(), &params, first, count), context.handle, "ct_baked_render_accumulate");
        }
        CtBake bake = nullptr, halfCopy = nullptr;
        CtGroupBake groupBake = nullptr;
    };

    // The reference's default renderer (BakedRenderer): the network evaluated once per light on a probe grid (ct_network_bake,
    // --net-baked NX,NY,NZ,NPHI,NC) and every subframe interpolated from that table (ct_baked_render_*): no gather and no
    // network per subframe.  The table is baked in init, which follows Sun::init and so every ct_set_light, and baked again
    // should the light have changed since.  With --gpus the table is built on the group (ct_group_network_bake) and every GPU
    // renders its own tiles from its copy (ct_group_baked_render_accumulate).  sparse (--net-bake-sparse): the
    // table is baked by ct_network_bake_sparse, only where a first flight can look it up; the images are the same.  compact
    // (--net-bake-compact): ct_network_bake_compact, which also stores only those probes; the images are the same again.
    class BakedRenderer : public NetworkRenderer
    {
    public:
        BakedRenderer(std::shared_ptr<Context> context, std::shared_ptr<const NetworkFile> file, const CtNetworkRender& params, const CtBakeDesc& desc,
                      bool sparse = false, bool compact = false, const BakeFiles& files = {}, uint32_t traceDepth = 0)
            : NetworkRenderer(std::move(context), std::move(file), params), desc(desc), sparse(sparse), compact(compact), files(files),
              traceDepth(traceDepth) {}

        void init() override
        {
            NetworkRenderer::init();
            CtBake& bake = table.bake;
            if (bake) return;
            if (context->group)
            {
                if (!table.load(*context, files))
                {
                    Context::checkGroup(ct_group_network_bake(context->group, groupNetwork, &desc, compact ? CT_BAKE_COMPACT : sparse ? CT_BAKE_SPARSE : CT_BAKE_DENSE,
                                                              &table.groupBake), context->group, "ct_group_network_bake");
                    table.adoptShard(*context);
                }
                table.finish(BakeHolder::handleOf(*context), files, true);
                return;
            }
            if (!table.load(context->handle, files))
            {
                if (compact) Context::check(ct_network_bake_compact(context->handle, network, &desc, &bake), context->handle, "ct_network_bake_compact");
                else if (sparse) Context::check(ct_network_bake_sparse(context->handle, network, &desc, &bake), context->handle, "ct_network_bake_sparse");
                else Context::check(ct_network_bake(context->handle, network, &desc, &bake), context->handle, "ct_network_bake");
            }
            table.finish(context->handle, files, true);
        }

        void render(float* frameResultBuffer) override
        {
            if (context->group) throw std::runtime_error("the two-launch loop (--unfused) renders on one GPU only");
            applyCamera();
            refresh();
            table.render(*context, params, traceDepth, subframeId, frameResultBuffer);
        }

        void renderAccumulate(uint32_t first, uint32_t count, bool /*enqueue: the call waits once, at its end*/) override
        {
            applyCamera();
            refresh();
            table.renderAccumulate(*context, params, traceDepth, first, count);
        }

    private:
        void refresh()   // a light set since the bake: bake again (and round again, with --bake-half)
        {
            const CtHandle handle = BakeHolder::handleOf(*context);
            if (table.current(handle)) return;
            if (context->group) Context::checkGroup(ct_group_bake_update(table.groupBake, groupNetwork), context->group, "ct_group_bake_update");
            else Context::check(ct_bake_update(context->handle, network, table.bake), context->handle, "ct_bake_update");
            table.finish(handle, files, false);
        }

        CtBakeDesc desc;
        bool sparse, compact;
        BakeFiles files;
        uint32_t traceDepth;   // --net-trace-depth K: hybrid frames of depth K (0: the table is read at the first collision)
        BakeHolder table;   // (destroyed before the network and the handle)
    };

    // The baked renderer without a network (--traced-bake NX,NY,NZ,NPHI,NC --bake-samples N): the probe table holds the means of
    // N experiments of the path tracer's point estimator per entry (ct_bake_traced) and every subframe is interpolated from it.
    // Traced in init, and again (ct_bake_retrace) should the light have changed since.  With --gpus the table is traced on the
    // group (ct_group_bake_traced, ct_group_bake_traced_adaptive) and every GPU renders its own tiles from its copy.
    // With --bake-adaptive R,MAX[,REL[,ABS[,ZERO]]] in place of --bake-samples the table is traced in rounds under the stopping rule
    // (ct_bake_traced_adaptive, ct_bake_retrace_adaptive) and init prints what ct_bake_adaptive_info reports.
    class TracedBakeRenderer : public PathTracingRenderer
    {
    public:
        TracedBakeRenderer(std::shared_ptr<Context> context, const CtNetworkRender& params, const CtBakeDesc& desc, uint32_t kind, uint32_t samples,
                           const CtBakeAdaptive* adaptive = nullptr, const BakeFiles& files = {}, uint32_t traceDepth = 0)
            : PathTracingRenderer(std::move(context)), params(params), desc(desc), kind(kind), samples(samples), isAdaptive(adaptive != nullptr),
              adaptive(adaptive ? *adaptive : CtBakeAdaptive{}), files(files), traceDepth(traceDepth) {}

        void init() override
        {
            PathTracingRenderer::init();
            CtBake& bake = table.bake;
            if (bake) return;
            const CtHandle handle = BakeHolder::handleOf(*context);
            if (table.load(*context, files))   // --bake-in: how to trace it again, should the light change, is the file's
            {
                CtBakeTraceInfo ti;
                CtBakeAdaptiveInfo ai;
                Context::check(ct_bake_trace_info(bake, &ti), handle, "ct_bake_trace_info");
                Context::check(ct_bake_adaptive_info(bake, &ai), handle, "ct_bake_adaptive_info");
                if (!ti.traced) throw std::runtime_error("--bake-in: the file holds a network's bake; give its network with --network FILE");
                samples = ti.samples;
                isAdaptive = ai.adaptive != 0;
            }
            else if (context->group)
            {
                if (!isAdaptive) Context::checkGroup(ct_group_bake_traced(context->group, &desc, kind, samples, &table.groupBake), context->group, "ct_group_bake_traced");
                else Context::checkGroup(ct_group_bake_traced_adaptive(context->group, &desc, kind, &adaptive, &table.groupBake), context->group, "ct_group_bake_traced_adaptive");
                table.adoptShard(*context);
            }
            else if (!isAdaptive) Context::check(ct_bake_traced(context->handle, &desc, kind, samples, &bake), context->handle, "ct_bake_traced");
            else Context::check(ct_bake_traced_adaptive(context->handle, &desc, kind, &adaptive, &bake), context->handle, "ct_bake_traced_adaptive");
            if (isAdaptive) printAdaptiveInfo();
            table.finish(handle, files, true);
        }

        void render(float* frameResultBuffer) override
        {
            if (context->group) throw std::runtime_error("the two-launch loop (--unfused) renders on one GPU only");
            applyCamera();
            refresh();
            table.render(*context, params, traceDepth, subframeId, frameResultBuffer);
        }

        void renderAccumulate(uint32_t first, uint32_t count, bool /*enqueue: the call waits once, at its end*/) override
        {
            applyCamera();
            refresh();
            table.renderAccumulate(*context, params, traceDepth, first, count);
        }

    private:
        void refresh()   // a light set since the bake: trace again (and round again, with --bake-half)
        {
            const CtHandle handle = BakeHolder::handleOf(*context);
            if (table.current(handle)) return;
            if (context->group)
            {
                if (!isAdaptive) Context::checkGroup(ct_group_bake_retrace(table.groupBake, samples), context->group, "ct_group_bake_retrace");
                else Context::checkGroup(ct_group_bake_retrace_adaptive(table.groupBake), context->group, "ct_group_bake_retrace_adaptive");
            }
            else if (!isAdaptive) Context::check(ct_bake_retrace(context->handle, table.bake, samples), context->handle, "ct_bake_retrace");
            else Context::check(ct_bake_retrace_adaptive(context->handle, table.bake), context->handle, "ct_bake_retrace_adaptive");
            if (isAdaptive) printAdaptiveInfo();
            table.finish(handle, files, false);
        }

        void printAdaptiveInfo()
        {
            CtBakeAdaptiveInfo i;
            Context::check(ct_bake_adaptive_info(table.bake, &i), BakeHolder::handleOf(*context), "ct_bake_adaptive_info");
            std::printf("adaptive bake: %u rounds of %u, cap %u; %llu entries, %llu converged, %llu capped, %llu paths; "
                        "trace %.3f ms, fold %.3f ms, test %.3f ms\n", i.rounds, i.round_samples, i.max_samples,
                        (unsigned long long)i.entries_active, (unsigned long long)i.converged, (unsigned long long)i.capped,
                        (unsigned long long)i.paths, i.trace_ms, i.fold_ms, i.test_ms);
        }

        CtNetworkRender params;
        CtBakeDesc desc;
        uint32_t kind, samples;
        bool isAdaptive;
        CtBakeAdaptive adaptive;
        BakeFiles files;
        uint32_t traceDepth;   // --net-trace-depth K, as in BakedRenderer
        BakeHolder table;   // (destroyed before the handle)
    };

    class Camera : public SceneItem                                              // Camera.h:16-103
    {
    public:
        struct Settings
        {
            Settings(uint32_t width, uint32_t height, std::filesystem::path outputFile)
                : width(width), height(height), outputFile(std::move(outputFile)) {}
            uint32_t width, height;
            std::filesystem::path outputFile;
        };

        Camera(std::shared_ptr<Settings> settings, std::shared_ptr<Context> context, std::shared_ptr<ARenderer> renderer)
            : width(settings->width), height(settings->height), outputFile(settings->outputFile),
              context(std::move(context)), renderer(std::move(renderer))
        {
            this->context->scene.width = width;
            this->context->scene.height = height;
        }

        void init() override                                                     // Camera.cpp:22-66
        {
            renderer->init();
            cameraEye = { 2.5f, -0.4f, 0.f };                                    // :37-39
            cameraLookat = { 0.f, 0.f, 0.f };
            cameraUp = { 0.f, 1.f, 0.f };
            updatePosition();
            reset();
        }

        void update() override { if (!isCompleted()) { updatePosition(); render(); } }   // :68-75

        void reset() override                                                    // :77-86
        {
            subframeId = 0;
            context->resetAccumulation();
            // headless: the test the reference makes before every update of 10 (:179, :232-268) runs on the device behind every
            // 10th subframe's accumulate kernel and freezes the image where the reference's loop would stop
            deviceStops = headless && fused && context->stopWhenConverged(subframesPerUpdate, 100);
        }

        bool isCompleted() override { return completed; }

        void setEye(const float3& eye) { cameraEye = eye; updatePosition(); reset(); }    // stands in for rotate(), :93-98
        void increaseExposure() { exposure *= 1.2f; }
        void decreaseExposure() { exposure /= 1.2f; }

        // How many subframes one render() call adds (10 in the reference, Camera.cpp:189) and when to stop
        // regardless of convergence (the reference runs until converged).
        uint32_t subframesPerUpdate = 10;
        uint32_t maxSubframes = 0;      // 0 = until isConverged()
        bool fused = true;              // one ct_render_accumulate per update instead of 2 launches per subframe
        bool headless = false;          // no display: enqueue the batches, read the buffers only where the reference saves
        bool completed = true;          // Camera.h:55

        bool deviceStops = false;       // the convergence test runs on the device (ct_set_stop_when_converged)

        // --adaptive: the image is an adaptive frame (ct_adaptive_frame_*) -- rounds that go only to the pixels which still fail
        // the test -- run to its end in one update; the handle's own image is not rendered.  adaptiveCountsFile: where the
        // per-pixel sample counts go, raw little-endian uint32, row-major (empty: nowhere).  On a context that is a group
        // (--adaptive-gpus) the frame is a CtGroupAdaptiveFrame: the same files and totals, from every GPU's own rounds.
        bool adaptive = false;
        CtAdaptiveFrameDesc adaptiveDesc{ CT_ABI_VERSION, 10, 100, 1000, 2e-2f, 1e-2f, 0, 0 };
        std::filesystem::path adaptiveCountsFile;

        uint32_t getSubframeId() const { return subframeId; }
        const std::vector<uint8_t>& getScreen() const { return screen; }

        void saveToDisk() const                                                  // :149-175
        {
            std::vector<float> mean((size_t)width * height * 4);
            context->downloadMean(mean.data(), mean.size() * sizeof(float));
            writeImage(mean);
        }

    private:
        void writeImage(const std::vector<float>& mean) const
        {
            std::cout << mean[((size_t)width * height / 2 + width / 2) * 4] << std::endl;   // :163
            if (outputFile.extension() == ".pfm")
            {
                // RGB float32, bottom row first, which is the buffer's own row order (row 0 = bottom)
                std::ofstream f(outputFile, std::ios::binary);
                f << "PF\n" << width << " " << height << "\n-1.0\n";
                for (size_t i = 0; i < (size_t)width * height; i++) f.write(reinterpret_cast<const char*>(&mean[4 * i]), 3 * sizeof(float));
            }
            else
            {
                // EXR, channels R, G, B FLOAT, DECREASING_Y, pixel (x, y) = progressive[y * width + x] like the reference
                Exr::writeRgbFloat(outputFile.string(), width, height, mean.data());
            }
        }

        void updatePosition()                                                    // :100-134 (arcball path is UI-only)
        {
            const float hfov = 30.0f;
            const float aspectRatio = static_cast<float>(width) / static_cast<float>(height);
            CameraProgram* camera = renderer->getCamera();
            if (camera != nullptr)
            {
                ct_calculate_camera_variables(cameraEye.data(), cameraLookat.data(), cameraUp.data(), hfov, aspectRatio,
                                              camera->U.data(), camera->V.data(), camera->W.data());
                camera->eye = cameraEye;
                camera->valid = true;
            }
        }

        // The whole job of --adaptive: create, update until nothing is live, save mean and counts, one line of totals.
        void renderAdaptive()
        {
            auto* pt = dynamic_cast<PathTracingRenderer*>(renderer.get());
            if (pt == nullptr || (context->group == nullptr && context->handle == nullptr)) throw std::runtime_error("--adaptive renders with the path tracer");
            pt->publishCamera();
            std::vector<float> mean((size_t)width * height * 4);
            std::vector<uint32_t> counts((size_t)width * height);
            CtAdaptiveFrameInfo info{};
            if (context->group) { renderAdaptiveGroup(mean, counts, info); finishAdaptive(mean, counts, info); return; }
            CtHandle h = context->handle;
            CtAdaptiveFrame frame = nullptr;
            Context::check(ct_adaptive_frame_create(h, &adaptiveDesc, &frame), h, "ct_adaptive_frame_create");
            int rc = ct_adaptive_frame_update(frame, 0);
            if (rc == CT_OK) rc = ct_adaptive_frame_info(frame, &info);
            if (rc == CT_OK) rc = ct_adaptive_frame_download(frame, CT_ADAPTIVE_MEAN, mean.data(), mean.size() * sizeof(float));
            if (rc == CT_OK) rc = ct_adaptive_frame_download(frame, CT_ADAPTIVE_COUNTS, counts.data(), counts.size() * sizeof(uint32_t));
            if (rc != CT_OK)
            {
                const std::string why = ct_last_error(h);   // (before the frame goes: destroy leaves the text alone, but keep it anyway)
                ct_adaptive_frame_destroy(frame);
                throw std::runtime_error("ct_adaptive_frame: " + why);
            }
            ct_adaptive_frame_destroy(frame);
            finishAdaptive(mean, counts, info);
        }

        // --adaptive-gpus: the same job on the context's group (ct_group_adaptive_frame_*) -- every shard runs its own rounds over
        // its own pixels, the merged mean and counts are the single handle's bytes -- and one line with every shard's paths and rounds.
        void renderAdaptiveGroup(std::vector<float>& mean, std::vector<uint32_t>& counts, CtAdaptiveFrameInfo& info)
        {
            CtGroup g = context->group;
            CtGroupAdaptiveFrame frame = nullptr;
            Context::checkGroup(ct_group_adaptive_frame_create(g, &adaptiveDesc, &frame), g, "ct_group_adaptive_frame_create");
            uint32_t shards = 0;
            std::ostringstream line;
            int rc = ct_group_adaptive_frame_update(frame, 0);
            if (rc == CT_OK) rc = ct_group_adaptive_frame_info(frame, &info);
            if (rc == CT_OK) rc = ct_group_adaptive_frame_download(frame, CT_ADAPTIVE_MEAN, mean.data(), mean.size() * sizeof(float));
            if (rc == CT_OK) rc = ct_group_adaptive_frame_download(frame, CT_ADAPTIVE_COUNTS, counts.data(), counts.size() * sizeof(uint32_t));
            if (rc == CT_OK) rc = ct_group_size(g, &shards);
            for (uint32_t i = 0; rc == CT_OK && i < shards; i++)
            {
                CtAdaptiveFrame shard = nullptr;
                CtAdaptiveFrameInfo s{};
                rc = ct_group_adaptive_frame_shard(frame, i, &shard);
                if (rc == CT_OK && ct_adaptive_frame_info(shard, &s) != CT_OK) rc = CT_E_INVAL;
                line << (i ? ", " : "") << "{\"pixels\": " << s.pixels << ", \"paths\": " << s.paths << ", \"rounds\": " << s.rounds << "}";
            }
            if (rc != CT_OK)
            {
                const std::string why = ct_group_last_error(g);
                ct_group_adaptive_frame_destroy(frame);
                throw std::runtime_error("ct_group_adaptive_frame: " + why);
            }
            ct_group_adaptive_frame_destroy(frame);
            std::cout << "adaptive_shards [" << line.str() << "]" << std::endl;
        }

        void finishAdaptive(const std::vector<float>& mean, const std::vector<uint32_t>& counts, const CtAdaptiveFrameInfo& info)
        {
            std::cout << "adaptive {\"rounds\": " << info.rounds << ", \"pixels\": " << info.pixels << ", \"converged\": " << info.converged
                      << ", \"capped\": " << info.capped << ", \"paths\": " << info.paths << "}" << std::endl;
            writeImage(mean);
            if (!adaptiveCountsFile.empty())
            {
                std::ofstream f(adaptiveCountsFile, std::ios::binary);
                f.write(reinterpret_cast<const char*>(counts.data()), (std::streamsize)(counts.size() * sizeof(uint32_t)));
                if (!f) throw std::runtime_error("cannot write " + adaptiveCountsFile.string());
            }
            completed = true;
        }

        void render()                                                            // :177-230
        {
            if (adaptive) { renderAdaptive(); return; }
            // headless: nobody looks at the screen between saves, so batches are enqueued (a launch hands its
            // unfinished paths to the next one instead of ending with a tail) and the buffers are only read --
            // tonemap, save -- every 40 subframes, where the reference saves (:211-214).  The reference tests convergence
            // before every update of 10 subframes: the device does that behind every 10th subframe (deviceStops) and freezes
            // the image at the count where the reference's loop stops; the host learns of it at the next save point, takes
            // that count and that image, and is done -- the subframes enqueued meanwhile were rendered and dropped.  (A group
            // of GPUs tests its merged frame at the save points only and may stop up to 30 subframes later.)
            const bool look = !headless || subframeId % 40 == 0;
            if (deviceStops && look && subframeId >= 100)
            {
                uint64_t left = 0;
                const uint32_t at = context->convergedAt(left);   // (the tonemap of this save point has waited for everything)
                if (at != 0)
                {
                    std::cout << "Converged: " << (uint64_t)width * height - left << "/" << (uint64_t)width * height << " --- " << left << "left" << std::endl;
                    subframeId = at;
                    completed = true;
                    std::cout << "rendering subframe " << subframeId << std::endl;
                    saveToDisk();
                    return;
                }
            }
            if (!(look && !deviceStops && isConverged()) && !(maxSubframes && subframeId >= maxSubframes))
            {
                // headless: one batch up to the next point where anything is read (at 1024^2 a batch of 40 costs 15.4 ms where
                // four of 10 cost 18.5: a short launch has every pixel group in flight at once and misses L2 half again as
                // often); results do not depend on the batching
                uint32_t count = headless ? 40 - subframeId % 40 : subframesPerUpdate;
                if (maxSubframes) count = std::min(count, maxSubframes - subframeId);
                auto* pt = dynamic_cast<PathTracingRenderer*>(renderer.get());
                if (fused && pt != nullptr)
                {
                    pt->renderAccumulate(subframeId + 1, count, headless);        // (the estimator's fused batch, or the network's)
                    subframeId += count;
                    std::cout << "rendering subframe " << subframeId << std::endl;
                }
                else
                {
                    for (uint32_t i = 0; i < count; i++)
                    {
                        subframeId++;
                        if (pt) pt->subframeId = subframeId;                      // context["subframeId"]->setUint, :192
                        std::cout << "rendering subframe " << subframeId << std::endl;
                        renderer->render(nullptr);                                // :195
                        Context::check(ct_accumulate(context->handle, subframeId, nullptr), context->handle, "ct_accumulate");   // :197-199
                    }
                }
                if (!headless || subframeId % 40 == 0)
                {
                    screen.resize((size_t)width * height * 4);
                    context->tonemap(exposure, screen.data());                    // :202-210
                }
                if (subframeId % 40 == 0) saveToDisk();                           // :211-214
            }
            else
            {
                if (deviceStops)
                {
                    // (the subframe limit came first -- or did it?  the image may have frozen since the last save point)
                    uint64_t left = 0;
                    context->wait();
                    const uint32_t at = context->convergedAt(left);
                    if (at != 0) subframeId = at;
                }
                completed = true;
                std::cout << "rendering subframe " << subframeId << std::endl;
                saveToDisk();
            }
        }

        bool isConverged()                                                       // :232-268 (evaluated on the device)
        {
            if (subframeId < 100) return false;
            uint64_t left = 0;
            const bool converged = context->isConverged(left);
            std::cout << "Converged: " << (uint64_t)width * height - left << "/" << (uint64_t)width * height << " --- " << left << "left" << std::endl;
            return converged;
        }

        uint32_t width, height;
        std::filesystem::path outputFile;
        std::shared_ptr<Context> context;
        std::shared_ptr<ARenderer> renderer;
        uint32_t subframeId = 0;
        float3 cameraUp{}, cameraLookat{}, cameraEye{};
        float exposure = 0.4f;                                                   // Camera.h:90
        std::vector<uint8_t> screen;
    };
}
