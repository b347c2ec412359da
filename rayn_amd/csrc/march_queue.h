// march_queue.h — what the five persistent march kernels share (k_extend, k_extend1, k_shadow, k_shadow1 in kernels.hip; k_shadow_bulb in march_bulb.h): the
// cursor of the persistent queue, the ray and shadow-job records, the segment in an SDF's frame, one step of TracedSDF::occluded, the sphere fold and the
// counter flush - and, first, the three wave helpers all of it is built from, which every other kernel of kernels.hip uses too.  Included inside the kernels'
// namespace (kernels.hip; preview.hip, for store_job alone).  Plain inline functions and two small structs; listings and clock: DESIGN.md "Persistent march kernels".
#pragma once

RD uint32_t lane_id() { return threadIdx.x & 63u; }
// this lane's bit of a wave-uniform 64-bit mask as a predicate: the mask itself becomes the exec mask / the select's condition, no vector instruction
RD bool lane_of(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }
// number of set bits of a 64-bit wave mask below this lane
RD uint32_t mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- 1. the queue cursor ---------------------------------------------------------------------------------------------------------------------------
// A wave takes the queue [0, n) in chunks of CHUNK entries, ONE atomic on the queue's head per chunk, and hands the entries of its chunk to the lanes that
// need one, in lane order.  Everything is wave-uniform.  Results are written by entry, so which wave wins which chunk never shows in the output.
struct QueueSlot { bool mine; uint32_t entry; }; // this lane gets an entry from the window (only lanes of `need` may use it), and which
struct QueueCursor {
    uint32_t cur = 0, end = 0; // the window: what is left of the wave's chunk
    bool exhausted = false;    // a claim found the head at or beyond n: nothing is left for this wave, ever
    bool endgame = false;      // the chunk in hand was claimed with fewer than endgame_entries entries left in the queue: the kernels that hoard spare rays stop
                               // hoarding - a spare held by a lane that is still inside a long march would wait while other lanes idle (k_extend1, k_shadow1:
                               // ENDGAME_ENTRIES; k_extend and k_shadow hoard nothing and pass nothing; k_shadow_bulb, x K, keeps its flags itself: march_bulb.h)
    // One atomic on the head: the next chunk becomes the window.  Returns the entries that were left in the queue, chunk included; 0: none, and no window.
    RD uint32_t take_chunk(uint32_t* head, uint32_t n) {
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(head, CHUNK);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= n) return 0;
        cur = base; end = min(base + CHUNK, n);
        return n - base;
    }
    // Claim the next chunk if the window is empty.  False: the queue is exhausted; an exhausted cursor never touches the head again (k_extend comes back here
    // in every trip of its tail).  k_shadow_bulb writes the same rule out around take_chunk (march_bulb.h, phase A): a change to it is a change to both.
    RD bool claim(uint32_t* head, uint32_t n, uint32_t endgame_entries = 0) {
        if (cur == end && !exhausted) {
            const uint32_t left = take_chunk(head, n);
            if (left == 0) exhausted = true; else endgame = left < endgame_entries;
        }
        return !exhausted;
    }
    // Hand the window out to the lanes of `need` (wave-uniform mask, not empty): the first `avail` of them in lane order take cur + rank, the cursor moves past
    // what was taken.  A window too small for all of `need` leaves the rest to the caller's next trip (claim, then fetch again).
    RD QueueSlot fetch(uint64_t need) {
        const uint32_t rank = mbcnt(need), avail = end - cur;
        const QueueSlot slot = QueueSlot{rank < avail, cur + rank};
        cur += min((uint32_t)__popcll(need), avail);
        return slot;
    }
};

// ---- 2. the shadow-job record --------------------------------------------------------------------------------------------------------------------
// Nee::job_geo[3 * idx ..]: 24 bytes = start.xy | start.z, end.x | end.yz, at idx = [sample * cap + slot] (k_shade_setup; the preview's rounds use their own
// stride).  Nee::job_ref lists the pending idx; the packet time of a moving SDF is per slot (Nee::t0[idx % cap]) and only read when a hitable is sequenced.
RD void store_job(float2* __restrict__ job_geo, size_t idx, f3 a, f3 b) {
    job_geo[3 * idx] = make_float2(a.x, a.y);
    job_geo[3 * idx + 1] = make_float2(a.z, b.x);
    job_geo[3 * idx + 2] = make_float2(b.y, b.z);
}
RD void load_job(const Nee& nee, const DScene& sc, uint32_t ref, f3* a, f3* b, float* t0) {
    const float2 j0 = nee.job_geo[3 * (size_t)ref], j1 = nee.job_geo[3 * (size_t)ref + 1], j2 = nee.job_geo[3 * (size_t)ref + 2];
    *a = f3{j0.x, j0.y, j1.x}; *b = f3{j1.y, j2.x, j2.y};
    *t0 = sc.anim_spheres ? nee.t0[ref % (uint32_t)nee.cap] : 0.0f;
}

// ---- 3. the segment a -> b in the frame of SDF h (TracedSDF::occluded works on start - origin, end - origin; the origin at the packet time is an extension,
// zero in the reference): start, unit direction, length
RD void sdf_segment(const DHitable& h, f3 a, f3 b, float t0, f3* start, f3* dir, float* max_dist) {
    const f3 origin = sphere_center(h, t0);
    *start = a - origin;
    const f3 d = (b - origin) - *start;
    *max_dist = mag(d);
    *dir = div_by_mag(d, *max_dist);
}

// ---- 4. one step of TracedSDF::occluded (src/sdf.rs:25-57) in its two-region form, for the evaluation `dist` at march distance t.  The march state of a
// segment is t and one word: the marches so far (MS_COUNT: max_vis_marches < 0xFFFF, validate()), MS_FIRST until the first evaluation, MS_NAN when that one
// was NaN.  Returns -1 keep marching, 0 occluded, 1 this SDF does not occlude.  (k_extend1 / k_shadow1 run the same test as straight-line mask code.)
constexpr uint32_t MS_FIRST = 1u << 16, MS_NAN = 1u << 17, MS_COUNT = 0xFFFFu;
RD int occluded_step(uint32_t& ms, float& t, float dist, float max_dist, float c0, float c1, uint32_t max_vis) {
    bool nan = (ms & MS_NAN) != 0;
    int res = -1;
    if (ms & MS_FIRST) {
        t = dist; nan = dist != dist; ms = nan ? MS_NAN : 0u;
        if (max_vis == 0) res = ((dist < 0.0001f) && !((dist > max_dist) || nan)) ? 0 : 1;
        else if ((t > max_dist) || nan) res = 1;
    } else {
        if (__builtin_fabsf(dist) < fmaxs(c0, c1 * t)) res = 0;
        else {
            t = t + dist; ms++;
            if ((ms & MS_COUNT) == max_vis || (t > max_dist) || nan) res = 1;
        }
    }
    return res;
}

// ---- 5. the sphere fold and the ray record ---------------------------------------------------------------------------------------------------------
// HitableStore::add_hits (src/hitable.rs:177-198) over the analytic spheres h[k_begin .. k_end): first-wins minimum into closest / id
RD void fold_spheres(const DScene& sc, uint32_t k_begin, uint32_t k_end, f3 o, f3 d, float t0, float& closest, uint32_t& id) {
    for (uint32_t k = k_begin; k < k_end; k++) {
        const float ts = sphere_hit(sc.h[k], o, d, closest, t0);
        if (ts < closest) { closest = ts; id = k; }
    }
}
// Pool::geo0 / geo1 of path P: origin, direction and, where asked for, the bits word (hit object | sample index << 8)
RD void load_ray(const Pool& pool, uint32_t P, f3* o, f3* d) {
    const float4 g0 = pool.geo0[P];
    const float2 g1 = *(const float2*)(&pool.geo1[P].x);
    *o = f3{g0.x, g0.y, g0.z}; *d = f3{g0.w, g1.x, g1.y};
}
RD void load_ray(const Pool& pool, uint32_t P, f3* o, f3* d, uint32_t* sbits) {
    const float4 g0 = pool.geo0[P], g1 = pool.geo1[P];
    *o = f3{g0.x, g0.y, g0.z}; *d = f3{g0.w, g1.x, g1.y}; *sbits = __float_as_uint(g1.w);
}

// ---- 6. a lane's evaluation counters into the frame's: [0] evaluations, [4] fold / orbit iterations of the kernel's class
template <bool COUNT>
RD void flush_evals(const EvalCtr& evals, unsigned long long* __restrict__ evals_out) {
    if (COUNT && evals.n) { atomicAdd(evals_out, (unsigned long long)evals.n); atomicAdd(evals_out + 4, (unsigned long long)evals.it); }
}
