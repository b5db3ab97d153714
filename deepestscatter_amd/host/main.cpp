// cloudtrace -- headless equivalent of the reference's entry point for the path-traced image:
// main (src/main.cpp:26-77) -> Tasks::renderCloud (ExecutionLoop/Tasks.cpp:49-112): two tasks, light
// "Side" then "Back", 512x256, 7000 m, output <cloud>.<Light>.PT.exr (Tasks.cpp:88-90; --format pfm for PFM).  The GLUT loop
// (GuiExecutionLoop.cpp:85-128) becomes a plain while(!scene->isCompleted()) scene->update().
//
//   cloudtrace <cloud> [--size WxH] [--spp N] [--mode total|multi|single] [--light Side|Back|Front]...
//              (several --light: one task each; the tasks after the first re-light the first one's renderer, ct_set_light)
//              [--size-m 7000] [--out DIR] [--data DIR] [--unfused] [--display] [--estimator march|delta] [--format exr|pfm]
//              [--tex-fixed8]   filter weights in 1.8 fixed point like the reference's texture unit (CT_FLAG_TEX_FIXED8)
//              [--gpus N | --gpus a,b,c]   one process, one shard of 8x8-pixel tiles per GPU, RCCL reduce of [mean | M2] (ct_group_*)
//              [--network FILE [--net-transform linear|expm1] [--net-scale r,g,b] [--net-direct]]   the job's subframes come from
//                               the scattering network in FILE (NetworkFile.h; ct_network_render_accumulate, with --gpus
//                               ct_group_network_render_accumulate: every GPU renders its own tiles) instead of the
//                               estimator; --net-direct adds the sun's single-scatter term (CT_NET_ADD_SINGLE_SCATTER), so that a
//                               network trained on the multiple-scatter labels gives the picture --mode total gives
//              [--net-baked NX,NY,NZ,NPHI,NC]   with --network: bake the network once per light on that probe grid (ct_network_bake)
//                               and interpolate every subframe from the table (ct_baked_render_accumulate); with --gpus the table is
//                               baked across the GPUs and every GPU renders its own tiles from its copy (ct_group_bake_*)
//              [--net-bake-sparse]              with --net-baked: bake only the probes a first flight can reach (ct_network_bake_sparse); the same images
//              [--net-bake-compact]             with --net-baked: bake and store only those probes (ct_network_bake_compact); the same images; not with --net-bake-sparse
//              [--traced-bake NX,NY,NZ,NPHI,NC --bake-samples N [--net-bake-sparse | --net-bake-compact] [--net-direct]]   without
//                               --network: fill that probe grid with N path-traced experiments per entry (ct_bake_traced) and
//                               interpolate every subframe from the table; --net-scale and --net-transform apply; with --gpus every GPU
//                               traces a span of the table's nodes (ct_group_bake_traced) and renders its own tiles
//              [--bake-adaptive R,MAX[,REL[,ABS[,ZERO]]]]   in place of --bake-samples: trace in rounds of R experiments, only the entries
//                               that fail the stopping rule (95 % interval below REL of the mean, default 0.02, or below ABS, default
//                               1e-4; a zero entry after ZERO experiments, default 100000), at most MAX each (ct_bake_traced_adaptive)
//              [--bake-out FILE]                with --net-baked or --traced-bake: save the table as a bake file (ct_bake_save; with --gpus shard 0's, which is the whole table)
//              [--bake-in FILE]                 in place of --net-baked / --traced-bake and their flags: render from the table in FILE
//                               (ct_bake_load); a traced file needs no network, a network's bake needs its --network FILE (a new light bakes it again)
//              [--net-trace-depth K]            with --net-baked, --traced-bake or --bake-in: a hybrid frame (ct_baked_render_hybrid_*) -- the path
//                               tracer's own path through its first K collisions (1 .. 64), their NEE terms added, and the table read at
//                               collision K; K >= 2 needs --net-direct; works with --gpus
//              [--bake-half]                    render from the binary16 copy of the table (ct_bake_half); with --bake-out that copy is saved; not with --gpus
//              [--adaptive R,MAX[,MIN[,REL[,ABS]]] [--adaptive-counts FILE]]   the image as an adaptive frame (ct_adaptive_frame_*):
//                               rounds of R subframes that go only to the pixels which still fail the stopping rule (tested from MIN
//                               samples on, default 100; 95 % interval below REL of the mean, default 0.02, or below ABS, default
//                               0.01), at most MAX per pixel; the EXR is the adaptive mean, FILE gets the per-pixel sample counts
//                               (raw little-endian uint32, row-major); one GPU, the path tracer: not with --gpus, --network,
//                               --traced-bake or --display
//              [--adaptive-gpus N | --adaptive-gpus a,b,c]   with --adaptive: the frame on a CtGroup (ct_group_adaptive_frame_*), every
//                               GPU running its own rounds over its own 8x8-pixel tiles; the same EXR, counts file and adaptive {...}
//                               line as without it, byte for byte, and one adaptive_shards [...] line with every shard's paths and rounds
//   <cloud> = file.vdb | procedural:<N>[:<seed>] | file.f32grid
//
//   cloudtrace collect <cloud>|@list.txt [--scene-id I] [--scenes N] [--jobs K] [--gpus ..] [--batch 2048] [--light L] [--size-m M] [--out DIR] [--data DIR] [--estimator ..] [--tex-fixed8] [--device-collector]
//              = Tasks::collect (Tasks.cpp:114-155) for one SceneSetup: the ScatterSample, Result and DisneyDescriptor
//              collectors one after the other over records [I * batch, (I + 1) * batch), written as flat tables;
//              --device-collector: the radiance collector's loop runs on the device (ct_collector_*), same tables
#include <atomic>
#include <chrono>
#include <cstring>
#include <fstream>
#include <functional>
#include <mutex>
#include <queue>
#include <sstream>
#include <thread>

#include "Cameras.h"
#include "Collectors.h"

using namespace DeepestScatter;

namespace
{
    enum class LightDirection { Front, Side, Back };

    float3 getLightDirection(LightDirection direction)                            // Tasks.cpp:52-65
    {
        switch (direction)
        {
        case LightDirection::Front: return { -0.586f, -0.766f, -0.271f };
        case LightDirection::Side: return { -0.03f, -0.25f, 0.8f };
        case LightDirection::Back: return { 0.586f, -0.766f, -0.271f };
        }
        throw std::invalid_argument("Unexpected direction");
    }

    const char* toString(LightDirection d)
    {
        return d == LightDirection::Front ? "Front" : d == LightDirection::Side ? "Side" : "Back";
    }

    struct Options
    {
        std::string cloud;
        uint32_t width = 512, height = 256;                                       // Tasks.cpp:49-50
        uint32_t spp = 0;                                                         // 0 = until converged
        Cloud::Rendering::Mode mode = Cloud::Rendering::Mode::SunAndSkyAllScatter;
        std::vector<LightDirection> lights = { LightDirection::Side, LightDirection::Back };   // Tasks.cpp:108-109
        float sizeM = 7000.f;                                                     // main.cpp:63
        std::string outDir = ".", dataDir, format = "exr";
        bool fused = true;
        bool display = false;                                                     // --display: tonemap + convergence test after every update, like the GUI
        int estimator = CT_EST_MARCH;                                             // --estimator delta: Woodcock tracking (not the reference's sampler)
        bool texFixed8 = false;                                                   // --tex-fixed8: CT_FLAG_TEX_FIXED8, the reference's texture-unit weights
        std::vector<int32_t> devices;                                             // --gpus N | --gpus a,b,c: pixel-tile shards, RCCL frame reduce (ct_group_*)
        std::string networkPath;                                                  // --network FILE: the scattering network renders instead of the estimator
        std::shared_ptr<const NetworkFile> network;                               // ... read and checked before anything is created
        CtNetworkRender networkRender{ CT_ABI_VERSION, CT_NET_OUT_LINEAR, { 1.f, 1.f, 1.f }, 0 };   // --net-transform, --net-scale
        bool netBaked = false;                                                    // --net-baked NX,NY,NZ,NPHI,NC: render from a baked probe table (BakedRenderer)
        CtBakeDesc bake{ CT_ABI_VERSION, { 0, 0, 0 }, 0, 0 };
        bool netBakeSparse = false;                                               // --net-bake-sparse: ct_network_bake_sparse in place of ct_network_bake
        bool netBakeCompact = false;                                              // --net-bake-compact: ct_network_bake_compact in place of ct_network_bake
        bool tracedBake = false;                                                  // --traced-bake NX,NY,NZ,NPHI,NC: the table of `bake` traced, no network (TracedBakeRenderer)
        uint32_t bakeSamples = 0;                                                 // --bake-samples N: experiments per entry of the traced bake
        bool bakeAdaptive = false;                                                // --bake-adaptive R,MAX[,REL[,ABS[,ZERO]]]: the traced bake in rounds under the stopping rule
        CtBakeAdaptive adaptive{ CT_ABI_VERSION, 0, 0, 100000, 2e-2f, 1e-4f };
        BakeFiles bakeFiles;                                                      // --bake-in FILE, --bake-out FILE, --bake-half
        bool adaptiveFrame = false;                                               // --adaptive R,MAX[,MIN[,REL[,ABS]]]: the image as an adaptive frame (Camera::adaptive)
        CtAdaptiveFrameDesc adaptiveDesc{ CT_ABI_VERSION, 0, 100, 0, 2e-2f, 1e-2f, 0, 0 };
        std::string adaptiveCounts;                                               // --adaptive-counts FILE: the per-pixel sample counts
        std::vector<int32_t> adaptiveDevices;                                     // --adaptive-gpus N | a,b,c: the adaptive frame on a CtGroup (ct_group_adaptive_frame_*)
        uint32_t traceDepth = 0;                                                  // --net-trace-depth K: hybrid frames of depth K from the table (0: ct_baked_render_*)
        bool netDirect = false;                                                   // --net-direct: CT_NET_ADD_SINGLE_SCATTER joins networkRender.transform
        bool collect = false;                                                     // `cloudtrace collect ...`
        int32_t sceneId = 0;
        uint32_t batch = 2048;                                                    // Tasks.cpp:137
        uint32_t scenes = 1;                                                      // --scenes N: N setups of the same cloud (lights cycle), ids from --scene-id
        uint32_t jobs = 1;                                                        // --jobs K: scene setups in flight at once
        bool deviceCollector = false;                                             // --device-collector: DeviceRadianceCollector in place of RadianceCollector
    };

    // One line of a scene-setup list = what a Persistance::SceneSetup record carries (cloud path, cloud size, light direction).
    struct SceneSetupLine
    {
        std::string cloud;
        float3 light{};
        float sizeM = 7000.f;
    };

    struct CollectTotals
    {
        double radianceDeviceMs = 0;
        uint64_t experiments = 0;
        uint32_t updates = 0;
    };

    // Tasks::collect (Tasks.cpp:114-155) for one scene setup, with the three collectors the dataset pipeline chains:
    // installSceneSetup(sceneSetup, cloudRoot, SunMultipleScatter, Mipmaps::On), BatchSettings(i * 2048, 2048), EmptyRenderer.
    // Fills `dataset` with the setup's records; returns its timing line.
    std::string collectOne(const Options& opt, const SceneSetupLine& setup, int32_t sceneId, int32_t device, Dataset& out, CollectTotals& totals)
    {
        using Clock = std::chrono::steady_clock;
        const auto msSince = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
        auto t0 = Clock::now();
        auto context = std::make_shared<Context>();
        context->devices = { device };
        if (opt.texFixed8) context->scene.flags |= CT_FLAG_TEX_FIXED8;
        auto resources = std::make_shared<Resources>(context);
        SceneDescription scene{
            Cloud{ Cloud::Rendering{ 1.0f / 512.f, Cloud::Rendering::Mode::SunMultipleScatter },
                   Cloud::Model{ setup.cloud, Cloud::Model::Mipmaps::On, Cloud::Model::Size{ Meter{ setup.sizeM } } } },
            DirectionalLight{ setup.light, Color{ 1, 1, 1 }, 1e6f } };
        auto sun = std::make_shared<Sun>(std::make_shared<DirectionalLight>(scene.light), context);
        auto cloud = std::make_shared<VDBCloud>(std::make_shared<Cloud::Model>(scene.cloud.model), context, resources);
        auto material = std::make_shared<CloudMaterial>(std::make_shared<Cloud::Rendering>(scene.cloud.rendering), context);
        Resources::loadMie(opt.dataDir, context->mie, context->choppedMie);
        for (const std::shared_ptr<SceneItem>& item : std::vector<std::shared_ptr<SceneItem>>{ sun, cloud, material }) item->init();
        const double loadMs = msSince(t0);                                        // the volume on the host, quantised (Resources.cpp:68-155)
        t0 = Clock::now();
        createCollectorHandle(*context, opt.estimator);
        const double createMs = msSince(t0);                                      // upload, bricks, clearance, shadow volume (VDBCloud::init)

        auto dataset = std::make_shared<Dataset>();
        dataset->batchAppend("SceneSetup", { Persistance::sceneSetup(setup.cloud, setup.sizeM, scene.light.direction.data()) }, sceneId);
        const BatchSettings settings((uint32_t)sceneId * opt.batch, opt.batch);
        std::shared_ptr<SceneItem> radianceItem;
        const RadianceTimings* radiance = nullptr;
        if (opt.deviceCollector)
        {
            auto c = std::make_shared<DeviceRadianceCollector>(context, dataset, settings);
            radianceItem = c;
            radiance = c.get();
        }
        else
        {
            auto c = std::make_shared<RadianceCollector>(context, dataset, settings);
            radianceItem = c;
            radiance = c.get();
        }
        std::vector<std::shared_ptr<SceneItem>> collectors{
            std::make_shared<ScatterSampleCollector>(context, dataset, settings, sceneId),
            radianceItem,
            std::make_shared<DisneyDescriptorCollector>(context, dataset, settings) };
        double phaseMs[3] = { 0, 0, 0 };
        for (size_t k = 0; k < collectors.size(); k++)                            // each is its own task in the reference: init, update until completed
        {
            t0 = Clock::now();
            collectors[k]->init();
            while (!collectors[k]->isCompleted()) collectors[k]->update();
            phaseMs[k] = msSince(t0);
        }
        out.merge(*dataset);
        totals.radianceDeviceMs += radiance->totalRenderMs;
        totals.experiments += radiance->totalExperiments;
        totals.updates += radiance->updates;
        // one line for tools/gpu_collect_bench.sh: where a scene setup's time goes (the reference prints only "MS/Render")
        std::ostringstream line;
        line << "collect_timings {\"scene_id\": " << sceneId << ", \"cloud\": \"" << setup.cloud << "\", \"device\": " << device << ", \"batch\": " << opt.batch
             << ", \"load_ms\": " << loadMs << ", \"create_ms\": " << createMs << ", \"scatter_samples_ms\": " << phaseMs[0] << ", \"radiance_ms\": " << phaseMs[1]
             << ", \"radiance_device_call_ms\": " << radiance->totalRenderMs << ", \"radiance_updates\": " << radiance->updates
             << ", \"radiance_experiments\": " << radiance->totalExperiments << ", \"descriptors_ms\": " << phaseMs[2] << "}";
        return line.str();
    }

    // The scene setups of one run: `collect <cloud>` = one setup from the command line; `collect @list.txt` = one per line,
    // "<cloud> <Side|Back|Front|x,y,z> [sizeM]" (what GenerateSceneSetups.py writes into the SceneSetup table).
    std::vector<SceneSetupLine> readSetups(const Options& opt)
    {
        std::vector<SceneSetupLine> setups;
        if (opt.cloud.empty() || opt.cloud[0] != '@')
        {
            for (uint32_t i = 0; i < std::max(1u, opt.scenes); i++)
                setups.push_back({ opt.cloud, normalize(getLightDirection(opt.lights[i % opt.lights.size()])), opt.sizeM });
            return setups;
        }
        std::ifstream f(opt.cloud.substr(1));
        if (!f) throw std::runtime_error("cannot open scene setup list " + opt.cloud.substr(1));
        std::string row;
        while (std::getline(f, row))
        {
            std::istringstream in(row);
            std::string cloud, light;
            if (!(in >> cloud) || cloud[0] == '#') continue;
            SceneSetupLine s{ cloud, normalize(getLightDirection(LightDirection::Side)), opt.sizeM };
            if (in >> light)
            {
                float3 d{};
                if (std::sscanf(light.c_str(), "%f,%f,%f", &d[0], &d[1], &d[2]) == 3) s.light = normalize(d);
                else s.light = normalize(getLightDirection(light == "Front" ? LightDirection::Front : light == "Back" ? LightDirection::Back : LightDirection::Side));
                in >> s.sizeM;
            }
            setups.push_back(s);
        }
        if (setups.empty()) throw std::runtime_error("no scene setups in " + opt.cloud.substr(1));
        return setups;
    }

    // Tasks::collect's loop over scene setups (Tasks.h:59-71, Tasks.cpp:125-150).  The reference runs them one after the
    // other; a setup's radiance collector is a chain of small dependent launches (an update cannot start before the host has
    // re-packed the tasks the previous one left unconverged) whose length is set by its deepest paths, not by the GPU's
    // throughput, so `--jobs K` keeps K setups in flight -- one host thread and one renderer handle each, their launches
    // overlap on the device -- and `--gpus` deals the setups to the GPUs round-robin (no exchange between them: the setups
    // are independent).  Records do not depend on either: every setup's seeds come from its own record ids.
    int collectScenes(const Options& opt)
    {
        using Clock = std::chrono::steady_clock;
        const std::vector<SceneSetupLine> setups = readSetups(opt);
        const std::vector<int32_t> devices = opt.devices.empty() ? std::vector<int32_t>{ 0 } : opt.devices;
        // with --gpus every listed GPU gets at least one worker (jobs < gpus would leave devices idle), and setup i runs on
        // device i mod gpus whichever worker takes it
        const uint32_t jobs = std::max(1u, std::min<uint32_t>(std::max<uint32_t>(opt.jobs, opt.devices.empty() ? 1u : (uint32_t)devices.size()),
                                                             (uint32_t)setups.size()));
        CollectorLog::quiet() = jobs > 1;
        Dataset dataset;
        CollectTotals totals;
        std::mutex lock;
        std::atomic<uint32_t> next{ 0 };
        std::string firstError;
        const auto t0 = Clock::now();
        const auto worker = [&](uint32_t)
        {
            for (uint32_t i = next++; i < setups.size(); i = next++)
            {
                try
                {
                    Dataset mine;
                    CollectTotals mineTotals;
                    const std::string line = collectOne(opt, setups[i], opt.sceneId + (int32_t)i, devices[i % devices.size()], mine, mineTotals);
                    std::lock_guard<std::mutex> g(lock);
                    dataset.merge(mine);
                    totals.radianceDeviceMs += mineTotals.radianceDeviceMs;
                    totals.experiments += mineTotals.experiments;
                    totals.updates += mineTotals.updates;
                    std::cout << line << std::endl;
                }
                catch (const std::exception& e)
                {
                    std::lock_guard<std::mutex> g(lock);
                    if (firstError.empty()) firstError = e.what();
                    next = (uint32_t)setups.size();                              // stop handing out setups
                }
            }
        };
        std::vector<std::thread> threads;
        for (uint32_t w = 1; w < jobs; w++) threads.emplace_back(worker, w);
        worker(0);
        for (auto& t : threads) t.join();
        if (!firstError.empty()) throw std::runtime_error(firstError);
        const double wallMs = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        const auto t1 = Clock::now();
        dataset.save(opt.outDir);
        const double saveMs = std::chrono::duration<double, std::milli>(Clock::now() - t1).count();
        std::cout << "wrote " << dataset.getRecordsCount("ScatterSample") << " ScatterSample, " << dataset.getRecordsCount("Result")
                  << " Result, " << dataset.getRecordsCount("DisneyDescriptor") << " DisneyDescriptor records to " << opt.outDir << std::endl;
        std::cout << "collect_totals {\"scene_setups\": " << setups.size() << ", \"jobs\": " << jobs << ", \"gpus\": " << devices.size() << ", \"wall_ms\": " << wallMs
                  << ", \"save_ms\": " << saveMs << ", \"scene_setups_per_hour\": " << setups.size() * 3.6e6 / wallMs << ", \"radiance_updates\": " << totals.updates
                  << ", \"radiance_experiments\": " << totals.experiments << ", \"Mexperiments_per_s\": " << totals.experiments / wallMs / 1e3
                  << ", \"ms_per_update\": " << wallMs / std::max(1u, totals.updates) << "}" << std::endl;
        return 0;
    }

    using LazyTask = std::function<std::shared_ptr<Scene>()>;

    // `context`: one per cloud.  The reference builds a whole context per task; here the tasks of one cloud differ in the sun
    // alone, so the second and later ones keep the first one's renderer and re-light it (Sun::init -> ct_set_light, then
    // Camera::reset) instead of uploading the density and rebuilding its layouts again.  Same images.
    LazyTask renderCloudSingleTask(const Options& opt, LightDirection lightDirection, std::shared_ptr<Context> context)   // Tasks.cpp:67-102
    {
        return [=]()
        {
            const bool relight = context->created();
            context->devices = opt.adaptiveDevices.empty() ? opt.devices : opt.adaptiveDevices;
            context->alwaysGroup = !opt.adaptiveDevices.empty();                 // (--adaptive-gpus 1 is a group of one)
            if (opt.texFixed8) context->scene.flags |= CT_FLAG_TEX_FIXED8;
            auto resources = std::make_shared<Resources>(context);
            // installSceneSetup (installers.cpp:65-105)
            const float3 direction = normalize(getLightDirection(lightDirection));
            SceneDescription scene{
                Cloud{ Cloud::Rendering{ 1.0f / 512.f, opt.mode },
                       Cloud::Model{ opt.cloud, Cloud::Model::Mipmaps::On, Cloud::Model::Size{ Meter{ opt.sizeM } } } },
                DirectionalLight{ direction, Color{ 1, 1, 1 }, 1e6f } };
            std::string stem = std::filesystem::path(opt.cloud).filename().string();
            std::replace(stem.begin(), stem.end(), ':', '_');
            auto outputPath = std::filesystem::path(opt.outDir) / (stem + "." + toString(lightDirection) + "." + PathTracingRenderer::NAME + "." + opt.format);
            // installFramework + installApp: Sun, VDBCloud, CloudMaterial, Camera in this order (installers.cpp:28-38)
            std::shared_ptr<PathTracingRenderer> renderer = opt.tracedBake ? std::make_shared<TracedBakeRenderer>(context, opt.networkRender, opt.bake,
                    opt.netBakeCompact ? CT_BAKE_COMPACT : opt.netBakeSparse ? CT_BAKE_SPARSE : CT_BAKE_DENSE, opt.bakeSamples,
                    opt.bakeAdaptive ? &opt.adaptive : nullptr, opt.bakeFiles, opt.traceDepth)
                : !opt.network ? std::make_shared<PathTracingRenderer>(context)
                : opt.netBaked ? std::make_shared<BakedRenderer>(context, opt.network, opt.networkRender, opt.bake, opt.netBakeSparse, opt.netBakeCompact, opt.bakeFiles, opt.traceDepth)
                               : std::make_shared<NetworkRenderer>(context, opt.network, opt.networkRender);
            renderer->estimator = opt.estimator;
            auto sun = std::make_shared<Sun>(std::make_shared<DirectionalLight>(scene.light), context);
            auto cloud = std::make_shared<VDBCloud>(std::make_shared<Cloud::Model>(scene.cloud.model), context, resources);
            auto material = std::make_shared<CloudMaterial>(std::make_shared<Cloud::Rendering>(scene.cloud.rendering), context);
            auto camera = std::make_shared<Camera>(std::make_shared<Camera::Settings>(opt.width, opt.height, outputPath), context, renderer);
            camera->completed = false;                                            // Tasks.cpp:97-98
            camera->maxSubframes = opt.spp;
            camera->fused = opt.fused;
            camera->headless = opt.fused && !opt.display;
            camera->adaptive = opt.adaptiveFrame;
            camera->adaptiveDesc = opt.adaptiveDesc;
            camera->adaptiveCountsFile = opt.adaptiveCounts;
            std::vector<std::shared_ptr<SceneItem>> items{ sun, cloud, material, camera };
            if (relight) items = { sun, material, camera };                       // the volume is on the device already
            return std::make_shared<Scene>(items, context, opt.dataDir);
        };
    }
}

int main(int argc, char* argv[])
{
    std::string onGroup;   // told before a failure's text when a bake was asked for on a group of GPUs
    try
    {
        Options opt;
        if (argc < 2) { std::cerr << "usage: cloudtrace <cloud> [--size WxH] [--spp N] [--mode total|multi|single] [--light L] [--size-m M] [--out DIR] [--data DIR] [--unfused] [--display] [--estimator march|delta] [--format exr|pfm] [--gpus N|a,b,c] [--tex-fixed8] [--network FILE [--net-transform linear|expm1] [--net-scale r,g,b] [--net-direct] [--net-baked NX,NY,NZ,NPHI,NC [--net-bake-sparse | --net-bake-compact]]] [--traced-bake NX,NY,NZ,NPHI,NC --bake-samples N [--net-bake-sparse | --net-bake-compact] [--net-direct]] [--net-trace-depth K] [--adaptive R,MAX[,MIN[,REL[,ABS]]] [--adaptive-counts FILE] [--adaptive-gpus N|a,b,c]] (--network, --net-baked and --traced-bake with --gpus: every GPU renders its own tiles; --bake-half: one GPU)\n"; return 2; }
        int first = 2;
        bool lightsGiven = false;
        opt.cloud = argv[1];
        if (opt.cloud == "collect")
        {
            if (argc < 3) throw std::invalid_argument("cloudtrace collect <cloud> ...");
            opt.collect = true;
            opt.cloud = argv[2];
            opt.lights = { LightDirection::Side };
            first = 3;
        }
        opt.dataDir = (std::filesystem::path(argv[0]).parent_path() / ".." / "data").string();
        for (int i = first; i < argc; i++)
        {
            const std::string a = argv[i];
            auto next = [&]() { if (i + 1 >= argc) throw std::invalid_argument("missing value for " + a); return std::string(argv[++i]); };
            if (a == "--size") { if (std::sscanf(next().c_str(), "%ux%u", &opt.width, &opt.height) != 2) throw std::invalid_argument("--size WxH"); }
            else if (a == "--spp") opt.spp = (uint32_t)std::stoul(next());
            else if (a == "--size-m") opt.sizeM = std::stof(next());
            else if (a == "--out") opt.outDir = next();
            else if (a == "--data") opt.dataDir = next();
            else if (a == "--unfused") opt.fused = false;
            else if (a == "--scene-id") opt.sceneId = std::stoi(next());
            else if (a == "--batch") opt.batch = (uint32_t)std::stoul(next());
            else if (a == "--scenes") opt.scenes = (uint32_t)std::stoul(next());
            else if (a == "--jobs") opt.jobs = (uint32_t)std::stoul(next());
            else if (a == "--device-collector") opt.deviceCollector = true;
            else if (a == "--gpus" || a == "--adaptive-gpus")
            {
                // "N" = devices 0..N-1; "a,b,c" = that list (a device may repeat: a rehearsal of N shards on fewer GPUs)
                const std::string v = next();
                std::vector<int32_t>& devices = a == "--gpus" ? opt.devices : opt.adaptiveDevices;
                devices.clear();
                if (v.find(',') == std::string::npos) { for (int d = 0; d < std::stoi(v); d++) devices.push_back(d); }
                else { size_t p = 0; while (p <= v.size()) { const size_t q = v.find(',', p); devices.push_back(std::stoi(v.substr(p, q - p))); if (q == std::string::npos) break; p = q + 1; } }
                if (devices.empty()) throw std::invalid_argument(a + " N | " + a + " a,b,c");
            }
            else if (a == "--display") opt.display = true;
            else if (a == "--network") opt.networkPath = next();
            else if (a == "--net-transform")
            {
                const std::string t = next();
                if (t == "linear") opt.networkRender.transform = CT_NET_OUT_LINEAR;
                else if (t == "expm1") opt.networkRender.transform = CT_NET_OUT_EXPM1;
                else throw std::invalid_argument("--net-transform linear|expm1");
            }
            else if (a == "--net-scale")
            {
                float* s = opt.networkRender.rgb_scale;
                if (std::sscanf(next().c_str(), "%f,%f,%f", &s[0], &s[1], &s[2]) != 3) throw std::invalid_argument("--net-scale r,g,b");
            }
            else if (a == "--net-direct") opt.netDirect = true;
            else if (a == "--net-trace-depth")
            {
                const long k = std::stol(next());
                if (k < 1 || k > 64) throw std::invalid_argument("--net-trace-depth K, 1 .. 64");
                opt.traceDepth = (uint32_t)k;
            }
            else if (a == "--net-baked")
            {
                CtBakeDesc& b = opt.bake;
                if (std::sscanf(next().c_str(), "%u,%u,%u,%u,%u", &b.grid[0], &b.grid[1], &b.grid[2], &b.azimuths, &b.cosines) != 5) throw std::invalid_argument("--net-baked NX,NY,NZ,NPHI,NC");
                opt.netBaked = true;
            }
            else if (a == "--traced-bake")
            {
                CtBakeDesc& b = opt.bake;
                if (std::sscanf(next().c_str(), "%u,%u,%u,%u,%u", &b.grid[0], &b.grid[1], &b.grid[2], &b.azimuths, &b.cosines) != 5) throw std::invalid_argument("--traced-bake NX,NY,NZ,NPHI,NC");
                opt.tracedBake = true;
            }
            else if (a == "--bake-samples")
            {
                const long n = std::stol(next());
                if (n < 1 || n > 65535) throw std::invalid_argument("--bake-samples N, 1 .. 65535");
                opt.bakeSamples = (uint32_t)n;
            }
            else if (a == "--bake-adaptive")
            {
                CtBakeAdaptive& p = opt.adaptive;
                if (std::sscanf(next().c_str(), "%u,%u,%f,%f,%u", &p.round_samples, &p.max_samples, &p.rel_tol, &p.abs_tol, &p.zero_samples) < 2) throw std::invalid_argument("--bake-adaptive R,MAX[,REL[,ABS[,ZERO]]]");
                opt.bakeAdaptive = true;
            }
            else if (a == "--adaptive")
            {
                CtAdaptiveFrameDesc& p = opt.adaptiveDesc;
                const int got = std::sscanf(next().c_str(), "%u,%u,%u,%f,%f", &p.round_samples, &p.max_samples, &p.min_samples, &p.rel_tol, &p.abs_tol);
                if (got < 2) throw std::invalid_argument("--adaptive R,MAX[,MIN[,REL[,ABS]]]");
                opt.adaptiveFrame = true;
            }
            else if (a == "--adaptive-counts") opt.adaptiveCounts = next();
            else if (a == "--net-bake-sparse")
            {
                opt.netBakeSparse = true;
            }
            else if (a == "--net-bake-compact")
            {
                opt.netBakeCompact = true;
            }
            else if (a == "--bake-in") opt.bakeFiles.in = next();
            else if (a == "--bake-out") opt.bakeFiles.out = next();
            else if (a == "--bake-half") opt.bakeFiles.half = true;
            else if (a == "--tex-fixed8") opt.texFixed8 = true;
            else if (a == "--estimator")
            {
                const std::string e = next();
                if (e == "march") opt.estimator = CT_EST_MARCH;
                else if (e == "delta") opt.estimator = CT_EST_DELTA;
                else throw std::invalid_argument("--estimator march|delta");
            }
            else if (a == "--format") { opt.format = next(); if (opt.format != "exr" && opt.format != "pfm") throw std::invalid_argument("--format exr|pfm"); }
            else if (a == "--mode")
            {
                const std::string m = next();
                if (m == "total") opt.mode = Cloud::Rendering::Mode::SunAndSkyAllScatter;
                else if (m == "multi") opt.mode = Cloud::Rendering::Mode::SunMultipleScatter;
                else if (m == "single") opt.mode = Cloud::Rendering::Mode::SunSingleScatter;
                else throw std::invalid_argument("Invalid Render Mode");           // CloudMaterial.cpp:62
            }
            else if (a == "--light")
            {
                // the first --light replaces the default pair, every further one adds a task for the same cloud
                const std::string l = next();
                if (!lightsGiven) opt.lights.clear();
                lightsGiven = true;
                opt.lights.push_back(l == "Front" ? LightDirection::Front : l == "Back" ? LightDirection::Back : LightDirection::Side);
            }
            else throw std::invalid_argument("unknown option " + a);
        }

        if (opt.collect) return collectScenes(opt);

        if (opt.netDirect) opt.networkRender.transform |= CT_NET_ADD_SINGLE_SCATTER;   // (after the loop: --net-transform may follow it)
        if (!opt.bakeFiles.in.empty())
        {
            if (opt.tracedBake || opt.netBaked || opt.bakeSamples != 0 || opt.bakeAdaptive || opt.netBakeSparse || opt.netBakeCompact)
                throw std::invalid_argument("--bake-in takes the table and its kind from FILE: it cannot be combined with --net-baked, --traced-bake, "
                                            "--bake-samples, --bake-adaptive, --net-bake-sparse or --net-bake-compact");
            if (opt.bakeFiles.in == opt.bakeFiles.out) throw std::invalid_argument("--bake-in and --bake-out name the same file");
            CtBakeFileInfo info;   // (no device: a malformed file stops here)
            if (ct_bake_file_info(opt.bakeFiles.in.c_str(), &info) != CT_OK) throw std::invalid_argument(std::string("--bake-in: ") + ct_last_error(nullptr));
            if (info.header.traced && !opt.networkPath.empty())
                throw std::invalid_argument("--bake-in: the file holds a traced bake, which renders without a network: drop --network");
            if (!info.header.traced && opt.networkPath.empty())
                throw std::invalid_argument("--bake-in: the file holds a network's bake: give its network with --network FILE");
            (info.header.traced ? opt.tracedBake : opt.netBaked) = true;
        }
        else if ((!opt.bakeFiles.out.empty() || opt.bakeFiles.half) && !opt.tracedBake && !opt.netBaked)
            throw std::invalid_argument("--bake-out and --bake-half work on the table of --net-baked, --traced-bake or --bake-in");
        if (opt.traceDepth != 0 && !opt.tracedBake && !opt.netBaked)
            throw std::invalid_argument("--net-trace-depth K traces K collisions before the table of --net-baked, --traced-bake or --bake-in is read");
        if (opt.traceDepth >= 2 && !opt.netDirect)
            throw std::invalid_argument("--net-trace-depth K with K >= 2 needs --net-direct: a hybrid frame is the path tracer's total, the first collision's term included");
        if (opt.tracedBake && !opt.networkPath.empty()) throw std::invalid_argument("--traced-bake fills the table with path-traced radiance: it cannot be combined with --network");
        if (opt.tracedBake && opt.netBaked) throw std::invalid_argument("--traced-bake and --net-baked are two ways to fill one table: give one of them");
        if (opt.bakeAdaptive && opt.bakeSamples != 0) throw std::invalid_argument("--bake-adaptive and --bake-samples are two ways to trace one table: give one of them");
        if (opt.bakeAdaptive && !opt.tracedBake) throw std::invalid_argument("--bake-adaptive sets the rounds of --traced-bake NX,NY,NZ,NPHI,NC");
        if (opt.tracedBake && opt.bakeSamples == 0 && !opt.bakeAdaptive && opt.bakeFiles.in.empty()) throw std::invalid_argument("--traced-bake needs --bake-samples N or --bake-adaptive R,MAX[,REL[,ABS[,ZERO]]]");
        if (opt.bakeSamples != 0 && !opt.tracedBake) throw std::invalid_argument("--bake-samples counts the experiments of --traced-bake NX,NY,NZ,NPHI,NC");
        if (opt.bakeFiles.half && !opt.devices.empty()) throw std::invalid_argument("--bake-half makes its binary16 copy on one GPU: it cannot be combined with --gpus");
        if (opt.netBakeCompact && !opt.netBaked && !opt.tracedBake) throw std::invalid_argument("--net-bake-compact chooses how --net-baked NX,NY,NZ,NPHI,NC bakes and stores its table");
        if (opt.netBakeCompact && opt.netBakeSparse) throw std::invalid_argument("--net-bake-compact and --net-bake-sparse are two ways to bake one table: give one of them");
        if (opt.netBakeSparse && !opt.netBaked && !opt.tracedBake) throw std::invalid_argument("--net-bake-sparse chooses how --net-baked NX,NY,NZ,NPHI,NC bakes its table");
        if (opt.netBaked && opt.networkPath.empty()) throw std::invalid_argument("--net-baked bakes the network of --network FILE");
        if ((opt.netBaked || opt.tracedBake) && opt.devices.size() > 1)
            onGroup = std::string(opt.netBaked ? "--net-baked" : "--traced-bake") + " with --gpus builds and renders its table on a group of " +
                      std::to_string(opt.devices.size()) + " GPUs: ";
        if (opt.adaptiveFrame && (!opt.devices.empty() || !opt.networkPath.empty() || opt.tracedBake || opt.display))
            throw std::invalid_argument("--adaptive renders with the path tracer on one GPU, headless: it cannot be combined with --gpus, --network, --traced-bake or --display");
        if (!opt.adaptiveDevices.empty() && !opt.adaptiveFrame) throw std::invalid_argument("--adaptive-gpus N|a,b,c names the GPUs of --adaptive R,MAX[,MIN[,REL[,ABS]]]");
        if (!opt.adaptiveCounts.empty() && !opt.adaptiveFrame) throw std::invalid_argument("--adaptive-counts FILE names where the counts of --adaptive R,MAX[,MIN[,REL[,ABS]]] go");
        if (!opt.networkPath.empty())
        {
            // read and checked against the header's formula here, before a renderer exists: a malformed file costs no device
            opt.network = std::make_shared<const NetworkFile>(NetworkFile::load(opt.networkPath));
            if (opt.network->aux != 1) throw std::invalid_argument("--network: the renderer feeds one aux input (the light angle); this network has " + std::to_string(opt.network->aux));
        }

        std::queue<LazyTask> tasks;                                               // Tasks::renderCloud, Tasks.cpp:104-112
        auto context = std::make_shared<Context>();
        for (auto l : opt.lights) tasks.push(renderCloudSingleTask(opt, l, context));

        while (!tasks.empty())                                                    // GuiExecutionLoop::getNextTask
        {
            auto scene = tasks.front()();
            tasks.pop();
            scene->init();
            while (!scene->isCompleted())                                         // glutDisplay, GuiExecutionLoop.cpp:114-128
            {
                const auto t1 = std::chrono::steady_clock::now();
                scene->update();
                const auto t2 = std::chrono::steady_clock::now();
                std::cout << "MS/FRAME " << std::chrono::duration<double, std::milli>(t2 - t1).count() << std::endl;
            }
        }
        return 0;
    }
    catch (const std::exception& e)                                               // main.cpp:65-76
    {
        std::cout << onGroup << e.what() << std::endl;
        return 1;
    }
}
