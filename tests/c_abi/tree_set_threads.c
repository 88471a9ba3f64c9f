/* mk_tree_set under threads (C99 + pthreads against include/prysm_merkle.h):
 * four threads each own a set, two threads share a fifth and update disjoint
 * halves of its lists; every final root must equal the root the same calls
 * give on one thread.  Prints the single-threaded roots ("root <set> <hex>",
 * tests/test_gpu_tree_set_threads.py holds them against the oracle) and
 * "ok: ..." on success.  Values are a formula of (set, index, round, byte). */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "prysm_merkle.h"

enum { N = 200, ROUNDS = 24, PER = 8, SETS = 5 };

#define CHK(x)                                                                   \
    do {                                                                         \
        mk_call* c_ = &call;                                                     \
        int rc_ = (x);                                                           \
        if (rc_ != MK_OK) {                                                      \
            fprintf(stderr, "%s: %d %s\n", #x, rc_, c_->err);                    \
            return rc_;                                                          \
        }                                                                        \
    } while (0)

static void value(uint8_t* out, uint32_t len, int set, uint64_t idx, int round) {
    for (uint32_t j = 0; j < len; ++j) out[j] = (uint8_t)(set * 31 + idx * 7 + round * 13 + j);
}

static int make_set(int set, mk_tree_set** out) {
    mk_call call = {-1, 0, {0}};
    uint32_t t = 0;
    uint8_t a_[N * 8], b_[N * 32], tail[8];
    CHK(mk_tree_set_new(&call, 72, out));
    CHK(mk_tree_set_add(&call, *out, MK_TREE_LIST, 8, NULL, 0, 0, 0, &t));
    CHK(mk_tree_set_add(&call, *out, MK_TREE_BYTES, 32, NULL, 0, 0, 32, &t));
    for (uint64_t i = 0; i < N; ++i) {
        value(a_ + 8 * i, 8, set, i, 200);
        value(b_ + 32 * i, 32, set, i, 201);
    }
    CHK(mk_tree_set_assign(&call, *out, 0, a_, N));
    CHK(mk_tree_set_assign(&call, *out, 1, b_, N));
    value(tail, 8, set, 0, 202);
    CHK(mk_tree_set_put(&call, *out, 64, tail, 8));
    return MK_OK;
}

/* ROUNDS rounds of PER updates to each tree inside [lo, hi), a root every fourth round */
static int run_ops(mk_tree_set* s, int set, uint64_t lo, uint64_t hi) {
    mk_call call = {-1, 0, {0}};
    uint64_t idx[PER];
    uint8_t a[PER * 8], b[PER * 32], root[32];
    for (int r = 0; r < ROUNDS; ++r) {
        for (int q = 0; q < PER; ++q) {
            idx[q] = lo + (uint64_t)(r * 5 + q * 3) % (hi - lo);
            value(a + 8 * q, 8, set, idx[q], r);
            value(b + 32 * q, 32, set, idx[q], r);
        }
        CHK(mk_tree_set_update(&call, s, 0, idx, a, PER));
        CHK(mk_tree_set_update(&call, s, 1, idx, b, PER));
        if (r % 4 == 3) CHK(mk_tree_set_root(&call, s, root));
    }
    return MK_OK;
}

struct job {
    mk_tree_set* s;
    int set;
    uint64_t lo, hi;
    int rc;
};

static void* worker(void* p) {
    struct job* j = (struct job*)p;
    j->rc = run_ops(j->s, j->set, j->lo, j->hi);
    return NULL;
}

int main(void) {
    mk_call call = {-1, 0, {0}};
    uint8_t want[SETS][32], got[32];
    mk_tree_set* s[SETS];
    /* one thread */
    for (int i = 0; i < SETS; ++i) {
        CHK(make_set(i + 1, &s[i]));
        if (i < 4) {
            CHK(run_ops(s[i], i + 1, 0, N));
        } else {
            CHK(run_ops(s[i], i + 1, 0, N / 2));
            CHK(run_ops(s[i], i + 1, N / 2, N));
        }
        CHK(mk_tree_set_root(&call, s[i], want[i]));
        printf("root %d ", i + 1);
        for (int b = 0; b < 32; ++b) printf("%02x", want[i][b]);
        printf("\n");
        mk_tree_set_free(s[i]);
    }
    /* six threads: four own a set each, two share the fifth */
    pthread_t th[6];
    struct job jobs[6];
    for (int i = 0; i < SETS; ++i) CHK(make_set(i + 1, &s[i]));
    for (int i = 0; i < 6; ++i) {
        jobs[i].s = s[i < 4 ? i : 4];
        jobs[i].set = (i < 4 ? i : 4) + 1;
        jobs[i].lo = i == 5 ? N / 2 : 0;
        jobs[i].hi = i == 4 ? N / 2 : N;
        jobs[i].rc = -1;
        if (pthread_create(&th[i], NULL, worker, &jobs[i]) != 0) return 2;
    }
    for (int i = 0; i < 6; ++i) pthread_join(th[i], NULL);
    for (int i = 0; i < 6; ++i)
        if (jobs[i].rc != MK_OK) return 3;
    int bad = 0;
    for (int i = 0; i < SETS; ++i) {
        CHK(mk_tree_set_root(&call, s[i], got));
        if (memcmp(got, want[i], 32) != 0) {
            printf("MISMATCH set %d\n", i + 1);
            bad = 1;
        }
        if (mk_tree_set_count(s[i], 0) != N || mk_tree_set_count(s[i], 1) != N) bad = 1;
        mk_tree_set_free(s[i]);
    }
    if (bad) return 1;
    printf("ok: 4 threads with a set each, 2 threads sharing one\n");
    return 0;
}
