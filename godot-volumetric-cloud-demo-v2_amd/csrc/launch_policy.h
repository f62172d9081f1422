// launch_policy.h -- which cloud kernel a launch runs, and how: variant, ray segments, workgroup order, cost feedback, persistent form.
// A pure function of the context's knobs and the launch size (no HIP): clouds_launch.cpp::clouds_dev calls it, and tests/hostsim compiles it
// with g++ so that tests/test_launch_policy.py pins every threshold on the CPU.  A wrong choice still renders a correct frame, only a slower one.
#pragma once

namespace csky {

struct LaunchKnobs {
    int variant;            // csky_set_variant
    bool cell32;            // exact cells are bound (csky_set_noise*)
    int segments;           // csky_set_segments: 0 = auto
    int sched_mode;         // csky_set_schedule: -1 = auto
    int frames_in_flight;   // csky_set_frames_in_flight
    int persistent;         // CSKY_PERSISTENT: 0 = never, 1 = the policy below, 2 = every whole-ray launch
};
struct LaunchPlan {
    int variant;            // the kernel that runs
    int seg;                // ray segments per ray (16: the "lds" variant's strip)
    int mode;               // workgroup order (7 = cost feedback)
    int static_mode;        // static order: the launch's own, or under feedback the first launch of a geometry's
    int bw;                 // workgroup footprint = bw x 8 pixels
    bool feedback;          // the kernel records per-workgroup costs and the next launch of the slot runs heaviest first
    bool persist;           // persistent launch form
};

// waves = wavefronts of whole rays in the launch (8 x 8 pixels each)
inline LaunchPlan plan_launch(const LaunchKnobs& k, long long waves) {
    // Launch-size policy: ray segments (more, shorter wavefronts) when the launch is too small to fill the chip with whole-ray
    // wavefronts, and the cost-feedback order (mode 7) when it is only a few resident workgroups deep.  Measured with
    // profiles/r01/launch_size_crossover_compact.txt (the script was retired with round 5's tools purge), "compact" variant, kernel ms at 256 / 1024 / 4096 / 8192 / 16384 / 32768 tiles of 8x8 rays
    // (= 1/128 .. 1/1 of the headline frame; profiles/r01/launch_size_crossover_compact.txt):
    //   whole rays, slab rows per XCD   (seg 1, sched 5)    0.50  0.56  0.58  0.94  1.39  2.15   <- full frames
    //   whole rays, cost feedback       (seg 1, sched 7)    0.50  0.51  0.66  0.80  1.10  2.18   <- 1/2 frame (one of 2 GPUs)
    //   2 step-range segments, feedback (seg 2, sched 7)    0.33  0.45  0.53  0.65  1.20  2.37   <- 1/4 frame
    //   4 step-range segments, feedback (seg 4, sched 7)    0.22  0.30  0.42  0.75  1.43  2.81   <- 1/8 frame
    //   4 step-range segments, natural  (seg 4, sched 2)    0.22  0.28  0.50  0.81  1.48  2.83
    //   4 interleaved segments, natural (seg 5, sched 2)    0.16  0.30  0.80  1.52  2.95  5.75   <- latency: the reference's 96x96 tiles
    // A lone wavefront is bound by its chain of dependent gathers, so small launches want more, shorter wavefronts; large
    // launches want the fewest instructions.  (The "queue" variant keeps its own, earlier crossovers: 6144 / 1536 wavefronts.)
    LaunchPlan p;
    const int variant = k.cell32 ? 3 : k.variant;                // exact cells exist for the compact whole-ray kernel only
    const bool queued = variant == 1 || variant == 3;
    int seg = k.cell32 ? 1 : (queued ? k.segments : 1);
    int auto_mode;
    // (the policy below is written for the kernel that RUNS: `variant`, not k.variant -- exact cells always march with the compact whole-ray kernel)
    if (variant == 3 && k.frames_in_flight >= 2) {
        // the caller keeps two frames in flight on two streams (csky_set_frames_in_flight): the next frame's workgroups fill this
        // launch's tail, so fewer, longer wavefronts win (tools/share_matrix.py, ms per frame at 1/2, 1/4, 1/8, 1/16 of the frame):
        //   seg 1: 0.96 (s5) 0.52 (s7) 0.42 0.35    seg 2: 1.18 0.61 0.34 (s7) 0.29    seg 4: 1.27 0.75 0.39 0.22 (s7)
        // With three or four frames in flight (the rings are four deep) a 1/8 share is best marched as whole rays:
        //   1/8 frame, cost feedback, x2 / x3 / x4:  seg 1 0.330 0.284 0.279   seg 2 0.313 0.352 0.355   (1/4 frame and larger: no gain over x2)
        // Round 4, rings eight deep (16 hardware queues): a 1/8 share x4 / x6 / x8: 0.247 / 0.228 / 0.224 ms (whole rays, static order; cost
        // feedback 0.242 / 0.226 / 0.222 once every ring slot has its previous launch's costs: not in a short run), a 1/4 share x2 / x4 / x8:
        // 0.487 / 0.446 / 0.415 static, 0.444 / 0.436 / 0.428 feedback; 1/2 and whole frames gain nothing beyond x2 (profiles/r04/frames_in_flight_depth.txt).
        const int whole_from = k.frames_in_flight >= 3 ? 3072 : 6144;
        if (queued && seg == 0) seg = waves >= whole_from ? 1 : (waves >= 3072 ? 2 : (waves >= 768 ? 4 : 5));
        auto_mode = (waves >= 12288 || (k.frames_in_flight >= 6 && waves >= 3072)) ? 5 : (waves >= 768 ? 7 : 2);
    } else if (variant == 3) {
        if (queued && seg == 0) seg = waves >= 12288 ? 1 : (waves >= 6144 ? 2 : (waves >= 768 ? 4 : 5));
        auto_mode = waves >= 24576 ? 5 : (waves >= 1536 ? 7 : 2);
    } else {
        if (queued && seg == 0) seg = waves >= 6144 ? 1 : (waves >= 1536 ? 4 : 5);
        auto_mode = waves >= 6144 ? 5 : 2;
    }
    if (variant == 2) seg = 16;
    int mode = k.sched_mode >= 0 ? k.sched_mode : auto_mode;
    p.bw = seg == 5 ? 8 : (seg == 16 ? 128 : 32 / seg);          // workgroup footprint = bw x 8 pixels (seg 5: one tile; seg 16: the 16-wavefront "lds" strip)
    p.feedback = mode == 7 && queued && seg != 5;                // kernels that record per-workgroup costs
    if (mode == 7 && !p.feedback) mode = waves >= 12288 ? 5 : 2;
    p.static_mode = mode == 7 ? (waves >= 12288 ? 5 : 2) : mode;   // order of the first launch of a geometry under feedback
    // Persistent launch form (cloud_kernels.hip::clouds_kernel_persistent): as many workgroups as the chip holds, their wavefronts pop
    // footprints from per-XCD sequences of the launch order and, at the end, from the other XCDs' sequences.  Measured
    // (profiles/r02/persistent_launch_ab.txt), ms per frame plain -> persistent: whole frame with two frames
    // in flight 1.806 -> 1.724 (bench.py, alternating runs), 1/2 frame 0.938 -> 0.882; one frame at a time 2.12 -> 2.17 (plain
    // launches refill freed slots at least as well when nothing else is in flight), 1/4 frame 0.477 -> 0.539 (barely deeper than
    // the resident grid), 4096x2048 6.13 -> 6.19 (no tail to fill), cost-feedback order 1.90 -> 2.09.  So: whole-ray launches of
    // 12 Ki to 64 Ki wavefronts (they run in the static XCD-row order) while the caller keeps two frames in flight.
    p.persist = !k.cell32 && seg == 1 && variant == 3 &&
                (k.persistent == 2 || (k.persistent == 1 && !p.feedback && k.frames_in_flight >= 2 && waves >= 12288 && waves <= 65536));
    p.variant = variant; p.seg = seg; p.mode = mode;
    return p;
}

}  // namespace csky
