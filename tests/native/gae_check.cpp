// gae_check — mev_gae.h's gae_step on the host: the text the device kernel (k_gae) compiles, run over
// (1) a hand-computed 3-step example, asserted here, and (2) fixed pseudo-random tables whose inputs and
// result bits are printed for tests/test_gae_ref.py, which runs actor_critic_ref.gae_ref on the printed
// inputs and compares bit for bit.  Built with -ffp-contract=off like the device tree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mev_gae.h"

namespace {

struct Case {
    const char* name;
    int T, E, N;
    float gamma, lambda;
    bool mask, has_done, has_term, has_trunc, has_eb;
    std::vector<float> r, v;
    std::vector<uint8_t> done, term, trunc, eb;
    std::vector<float> adv, ret;
    std::vector<uint8_t> valid;
};

uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// the scan of mev_gae (include/marlenv.h) around gae_step: per (e, i), t descending
void run(Case& c) {
    const size_t EN = size_t(c.E) * c.N;
    c.adv.assign(c.T * EN, 0.0f);
    c.ret.assign(c.T * EN, 0.0f);
    c.valid.assign(c.T * EN, 0);
    const float cc = c.gamma * c.lambda;
    for (int e = 0; e < c.E; ++e)
        for (int i = 0; i < c.N; ++i) {
            const size_t g = size_t(e) * c.N + i;
            float adv_next = 0.0f;
            for (int t = c.T - 1; t >= 0; --t) {
                const uint8_t d = c.has_done ? c.done[t * EN + g] : 0;
                const uint8_t te = c.has_term ? c.term[size_t(t) * c.E + e] : 0;
                const uint8_t tr = c.has_trunc ? c.trunc[size_t(t) * c.E + e] : 0;
                bool masked = false;
                if (c.mask) {
                    if (t > 0)
                        masked = ((c.has_term ? c.term[size_t(t - 1) * c.E + e] : 0) |
                                  (c.has_trunc ? c.trunc[size_t(t - 1) * c.E + e] : 0)) != 0;
                    else
                        masked = c.has_eb && c.eb[e] != 0;
                }
                const mev::GaeRow o = mev::gae_step(c.r[t * EN + g], c.v[t * EN + g], c.v[(t + 1) * EN + g], d, te, tr,
                                                    masked, c.gamma, cc, adv_next);
                c.adv[t * EN + g] = o.adv;
                c.ret[t * EN + g] = o.ret;
                c.valid[t * EN + g] = o.valid;
                adv_next = o.adv;
            }
        }
}

uint32_t g_rng = 0x2545F491u;
uint32_t next() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;  // 24 bits
}
float uniform(float lo, float hi) { return lo + (hi - lo) * (float(next()) * (1.0f / 16777216.0f)); }

Case table(const char* name, int T, int E, int N, float gamma, float lambda, bool mask, bool hd, bool hte, bool htr,
           bool heb) {
    Case c{name, T, E, N, gamma, lambda, mask, hd, hte, htr, heb, {}, {}, {}, {}, {}, {}, {}, {}, {}};
    const size_t EN = size_t(E) * N;
    for (size_t k = 0; k < T * EN; ++k) c.r.push_back(uniform(-2.0f, 2.0f));
    for (size_t k = 0; k < (T + 1) * EN; ++k) c.v.push_back(uniform(-30.0f, 30.0f));
    for (size_t k = 0; k < T * EN; ++k) c.done.push_back(next() % 5 == 0);
    for (size_t k = 0; k < size_t(T) * E; ++k) c.term.push_back(next() % 6 == 0);
    for (size_t k = 0; k < size_t(T) * E; ++k) c.trunc.push_back(next() % 4 == 0);  // (also together with term / done)
    for (int e = 0; e < E; ++e) c.eb.push_back(next() % 2);
    return c;
}

void print_f(const char* tag, const std::vector<float>& a) {
    printf("%s", tag);
    for (float x : a) printf(" %08x", bits(x));
    printf("\n");
}
void print_b(const char* tag, bool has, const std::vector<uint8_t>& a) {
    printf("%s", tag);
    if (!has) printf(" -");
    else
        for (uint8_t x : a) printf(" %u", unsigned(x));
    printf("\n");
}
void print(const Case& c) {
    printf("CASE %s %d %d %d %08x %08x %d\n", c.name, c.T, c.E, c.N, bits(c.gamma), bits(c.lambda), int(c.mask));
    print_f("R", c.r);
    print_f("V", c.v);
    print_b("D", c.has_done, c.done);
    print_b("TE", c.has_term, c.term);
    print_b("TR", c.has_trunc, c.trunc);
    print_b("EB", c.has_eb, c.eb);
    print_f("ADV", c.adv);
    print_f("RET", c.ret);
    print_b("VALID", true, c.valid);
}

int g_bad = 0;
void expect(const char* what, const Case& c, const float (&adv)[3], const float (&ret)[3], const uint8_t (&valid)[3]) {
    for (int t = 0; t < 3; ++t)
        if (bits(c.adv[t]) != bits(adv[t]) || bits(c.ret[t]) != bits(ret[t]) || c.valid[t] != valid[t]) {
            printf("MISMATCH %s t=%d: adv %a (want %a) ret %a (want %a) valid %d (want %d)\n", what, t, c.adv[t], adv[t],
                   c.ret[t], ret[t], int(c.valid[t]), int(valid[t]));
            ++g_bad;
        }
}

// r = 1, 2, 3; V = 0.5, 1, 1.5, 2; gamma = lambda = 0.5, c = 0.25: every figure below is exact in f32
Case hand(bool mask) {
    Case c{"hand", 3, 1, 1, 0.5f, 0.5f, mask, true, true, true, true, {1.0f, 2.0f, 3.0f}, {0.5f, 1.0f, 1.5f, 2.0f},
           {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0}, {}, {}, {}};
    return c;
}

}  // namespace

int main() {
    {  // no end: delta = 1, 1.75, 2.5; adv_2 = 2.5, adv_1 = 1.75 + 0.25 * 2.5, adv_0 = 1 + 0.25 * 2.375
        Case c = hand(false);
        run(c);
        expect("plain", c, {1.59375f, 2.375f, 2.5f}, {2.09375f, 3.375f, 4.0f}, {1, 1, 1});
    }
    {  // truncated at t = 1: bootstraps (delta_1 = 1.75) and cuts; adv_0 = 1 + 0.25 * 1.75; the mask zeroes row 2
        Case c = hand(false);
        c.trunc[1] = 1;
        run(c);
        expect("truncated", c, {1.4375f, 1.75f, 2.5f}, {1.9375f, 2.75f, 4.0f}, {1, 1, 1});
        c.mask = true;
        run(c);
        expect("truncated, masked", c, {1.4375f, 1.75f, 0.0f}, {1.9375f, 2.75f, 1.5f}, {1, 1, 0});
    }
    {  // terminated at t = 1: no bootstrap (delta_1 = 2 - 1), cut; adv_0 = 1 + 0.25 * 1
        Case c = hand(false);
        c.term[1] = 1;
        run(c);
        expect("terminated", c, {1.25f, 1.0f, 2.5f}, {1.75f, 2.0f, 4.0f}, {1, 1, 1});
    }
    {  // the agent's own done at t = 1: as a termination for this agent, and nothing is masked (the env runs on)
        Case c = hand(true);
        c.done[1] = 1;
        run(c);
        expect("done", c, {1.25f, 1.0f, 2.5f}, {1.75f, 2.0f, 4.0f}, {1, 1, 1});
    }
    {  // ended_before: row 0 is a reset step; done and truncated on the last row: stop wins (delta_2 = 3 - 1.5)
        Case c = hand(true);
        c.eb[0] = 1;
        c.done[2] = 1;
        c.trunc[2] = 1;
        run(c);
        expect("ended before", c, {0.0f, 2.125f, 1.5f}, {0.5f, 3.125f, 3.0f}, {0, 1, 1});
    }
    if (g_bad) {
        printf("GAE CHECK FAILED (%d)\n", g_bad);
        return 1;
    }
    const float gammas[2] = {0.99f, 1.0f}, lambdas[3] = {0.0f, 0.95f, 1.0f};
    int n = 0;
    for (float gamma : gammas)
        for (float lambda : lambdas)
            for (int opt = 0; opt < 4; ++opt) {
                // opt 0: no optional array; 1: all, masked; 2: done + truncated, masked without ended_before; 3: terminated only
                const bool all = opt == 1;
                Case c = table("table", 1 + (n * 5) % 13, 2 + n % 3, 1 + n % 4, gamma, lambda, opt == 1 || opt == 2,
                               all || opt == 2, all || opt == 3, all || opt == 2, all);
                run(c);
                print(c);
                ++n;
            }
    printf("GAE CHECK OK %d\n", n);
    return 0;
}
