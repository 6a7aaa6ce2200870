// rollout_sched_main.cpp -- stand-alone check of csrc/rollout_sched.h, the one statement of the device environment loop's cadence, against an independent law: the
// reference's own loop (src/solver.jl:134-145) walked ONE ENV STEP AT A TIME for the env-step cadence, `t % f == 0` for the vector-step cadence.  The unit chooser
// is held to soundness against that same per-step law.  Built with -fsanitize=address,undefined and run directly by tests/test_rollout_sched_cpu.py.  No HIP.
#include <stdio.h>
#include <string.h>
#include "rollout_sched.h"

static int g_errors = 0;
static long long g_checks = 0, g_cycles = 0, g_envcs = 0;
#define CHECK(c, ...) do { g_checks++; if (!(c)) { if (g_errors++ < 20) { fprintf(stderr, "%s:%d: CHECK failed: %s  [", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "]\n"); } } } while (0)

// the independent law: what runs behind vector step t of n copies
static RollDue law(int envc, long long t, long long n, long long tf, long long tu) {
    RollDue d = {0, false};
    if (envc) {      // the reference's loop: global env steps (t-1)*n+1 .. t*n, each tested on its own
        for (long long g = (t - 1) * n + 1; g <= t * n; g++) {
            if (tf > 0 && g % tf == 0) d.due++;
            if (tu > 0 && g % tu == 0) d.sync = true;
        }
    } else {
        if (tf > 0 && t % tf == 0) d.due = 1;
        if (tu > 0 && t % tu == 0) d.sync = true;
    }
    return d;
}

static const long long NS[] = {1, 3, 4, 8, 1024};
static const int TFS[] = {0, 1, 2, 3, 4, 7, 16, 17}, TUS[] = {0, 1, 5, 6, 25};

static dqn_rollout_cfg cfg_of(int envc, int tf, int tu, long long t0) {
    dqn_rollout_cfg c; memset(&c, 0, sizeof c);
    c.train_freq = tf; c.target_update_freq = tu; c.cadence_env_steps = envc; c.t0 = t0; c.eps_start = 1.0f; c.eps_stop = 0.1f; c.eps_steps = 100.0f;
    return c;
}

static void test_due() {
    for (int envc = 0; envc < 2; envc++) for (long long n : NS) for (int tf : TFS) for (int tu : TUS) for (long long t = 1; t <= 40; t++) {
        const dqn_rollout_cfg c = cfg_of(envc, tf, tu, t);      // (t0 does not enter: the law is a function of t)
        const RollDue a = rollout_due(c, t, n), b = law(envc, t, n, tf, tu);
        CHECK(a.due == b.due && a.sync == b.sync, "envc %d n %lld tf %d tu %d t %lld: header (%lld, %d), law (%lld, %d)", envc, n, tf, tu, t, a.due, (int)a.sync, b.due, (int)b.sync);
    }
}

// every unit the chooser picks is sound against the per-step law; CYCLE and ENVC are never picked for a recurrent engine, without graphs, or beyond the call's end
static void test_unit() {
    const long long SIZES[] = {0, 5, 60, 64, 4096}, LEFTS[] = {1, 2, 3, 4, 7, 16, 17, 40};
    for (int envc = 0; envc < 2; envc++) for (long long n : NS) for (int tf : TFS) for (int tu : TUS) for (long long t = 1; t <= 40; t++)
    for (int bits = 0; bits < 16; bits++) for (long long size : SIZES) for (long long left : LEFTS) {
        const dqn_rollout_cfg c = cfg_of(envc, tf, tu, t);
        RollFacts f; f.graph = bits & 1; f.single = bits & 2; f.tiny = bits & 4; f.rec = bits & 8; f.n = n; f.left = left; f.size = size; f.cap = 4096; f.B = 64;
        const RollUnit u = rollout_unit(c, t, f);
        if (u == ROLL_PLAIN) continue;
        CHECK(!f.rec && f.graph && f.single, "unit %d with rec %d graph %d single %d", (int)u, (int)f.rec, (int)f.graph, (int)f.single);
        if (u == ROLL_CYCLE) {
            g_cycles++;
            const long long F = rollout_cycle_len(c);
            CHECK(!envc && F >= 2 && F <= left, "cycle of %lld at t %lld with %lld steps left, envc %d", F, t, left, envc);
            for (long long s = t; s < t + F; s++) {
                const RollDue d = law(envc, s, n, tf, tu); const bool last = s == t + F - 1;
                CHECK(last || !d.sync, "tf %d tu %d t %lld: a sync at step %lld inside the cycle", tf, tu, t, s);
                CHECK(d.due == (last && tf > 0 ? 1 : 0), "tf %d tu %d t %lld: %lld train steps at step %lld of the cycle", tf, tu, t, d.due, s);
            }
            CHECK(tf == 0 || (size + F * n < 4096 ? size + F * n : 4096) >= 64, "cycle with the replay short of a batch at its last step (size %lld, F %lld, n %lld)", size, F, n);
        } else {
            g_envcs++;
            CHECK(u == ROLL_ENVC && envc && left >= 1 && !f.tiny && tf > 0, "unit %d envc %d left %lld tiny %d tf %d", (int)u, envc, left, (int)f.tiny, tf);
            const RollDue d = law(envc, t, n, tf, tu);
            CHECK(tf > 0 && n % tf == 0 && d.due == n / tf, "n %lld tf %d t %lld: the law gives %lld train steps, the graph holds n / train_freq", n, tf, t, d.due);
            CHECK((size + n < 4096 ? size + n : 4096) >= 64, "env-cadence graph with the replay short of a batch (size %lld, n %lld)", size, n);
        }
    }
    CHECK(g_cycles > 0 && g_envcs > 0, "the sweep chose %lld cycles and %lld env-cadence graphs", g_cycles, g_envcs);      // (both units occur: the soundness claims are not vacuous)
}

int main() {
    test_due(); test_unit();
    if (g_errors) { fprintf(stderr, "%d of %lld checks failed\n", g_errors, g_checks); return 1; }
    printf("rollout_sched OK: %lld checks, %lld cycles, %lld env-cadence graphs\n", g_checks, g_cycles, g_envcs);
    return 0;
}
