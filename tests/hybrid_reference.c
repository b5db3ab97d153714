/* The reference of tests/test_baked_hybrid.py for a hybrid frame's traced part (include/cloudtrace.h, "hybrid frames"): the
 * loop of the definition on the oracle's OWN free_flight, in_scattering, new_direction, intersect_box and ctx_init -- this file
 * includes the oracle's source, so their static definitions are the ones that run, not a restatement.  TEST INFRASTRUCTURE
 * ONLY; the test compiles it into its temporary directory with the flags of oracle/Makefile (and a second time with
 * -DORC_TEX_FIXED8).  Nothing under oracle/ changes. */
#include "../oracle/ct_oracle.c"

/* For every pixel (row 0 = bottom, as orc_render_subframe): hit = the primary ray met the box; state = 0 no collision (a miss,
 * or a first flight without a collision inside the box), 1 alive at collision `depth`, 2 ended before it; x_k = the position of
 * collision `depth` in world space (the flight's position - half box) and omega = the direction the path reached it along, both
 * of alive pixels only (0 otherwise); S = the sum of the NEE terms, from (0, 0, 0), in the path tracer's order.  The flight is
 * the march flight whatever s->estimator says. */
ORC_API void hybrid_reference_frame(const OrcScene *s, uint32_t subframe_id, uint32_t depth, uint8_t *hit, int32_t *state, float *x_k,
                                    float *omega, float *S)
{
    Ctx c;
    ctx_init(&c, s);
    c.estimator = 0;
    const v3 eye = v3_make(s->eye[0], s->eye[1], s->eye[2]);
    const v3 U = v3_make(s->U[0], s->U[1], s->U[2]);
    const v3 V = v3_make(s->V[0], s->V[1], s->V[2]);
    const v3 W = v3_make(s->W[0], s->W[1], s->W[2]);
    for (uint32_t py = 0; py < s->height; py++) {
        for (uint32_t px = 0; px < s->width; px++) {
            const size_t at = (size_t)py * s->width + px;
            OrcCounters k = { 0, 0, 0, 0, 0, 0 };
            const float dx = (float)px / (float)s->width * 2.f - 1.f;
            const float dy = (float)py / (float)s->height * 2.f - 1.f;
            const v3 ray_dir = v3_normalize(v3_add(v3_add(v3_scale(U, dx), v3_scale(V, dy)), W));
            uint32_t seed = orc_tea4(px * 4096u + py, subframe_id);
            v3 sum = v3_make(0, 0, 0), pos = v3_make(0, 0, 0), direction = v3_make(0, 0, 0);
            int32_t st = 0;
            float t_hit;
            hit[at] = (uint8_t)intersect_box(&c, eye, ray_dir, &t_hit);
            if (hit[at]) {
                pos = v3_add(eye, v3_scale(ray_dir, t_hit));
                pos = v3_add(pos, v3_scale(c.bbox, 0.5f));
                direction = v3_normalize(ray_dir);
                if (in_box(&c, pos)) {   /* (radiance_of_ray's loop condition before the first flight) */
                    const Event e = free_flight(&c, &seed, pos, direction, &k);
                    if (e.scattered && in_box(&c, e.pos)) {
                        pos = e.pos;
                        st = 1;
                    }
                }
            }
            for (uint32_t i = 1; st == 1; i++) {
                sum = v3_add(sum, in_scattering(&c, pos, direction, i != 1, &k));
                if (i == depth) {
                    break;
                }
                direction = new_direction(&c, &seed, direction);
                const Event e = free_flight(&c, &seed, pos, direction, &k);
                if (e.scattered && in_box(&c, e.pos)) {
                    pos = e.pos;
                } else {
                    st = 2;
                }
            }
            const v3 world = st == 1 ? v3_sub(pos, v3_scale(c.bbox, 0.5f)) : v3_make(0, 0, 0);
            const v3 w = st == 1 ? direction : v3_make(0, 0, 0);
            state[at] = st;
            x_k[3 * at + 0] = world.x; x_k[3 * at + 1] = world.y; x_k[3 * at + 2] = world.z;
            omega[3 * at + 0] = w.x; omega[3 * at + 1] = w.y; omega[3 * at + 2] = w.z;
            S[3 * at + 0] = sum.x; S[3 * at + 1] = sum.y; S[3 * at + 2] = sum.z;
        }
    }
}
