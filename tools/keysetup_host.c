/* keysetup_host.c -- the host side of tools/keysetup_bench.py (which compiles and runs it): the
 * per-key CPU baselines of the batched key setup, and the wall-clock batcher leg, in C so that no
 * interpreter overhead sits inside a timed loop.
 *
 *   keysetup_host N_RC4 N_BF N_CONN THREADS REPS
 *
 *   rc4_init_loop     BRB_RC4_Init of N_RC4 16-byte keys, one thread
 *   bf_init_loop      BRB_Blowfish_Init of N_BF 16-byte keys on 1 and on THREADS threads
 *   enable_loop       BRB_TransformBatcherEnable for N_CONN connections, one call each
 *   enable_batch      BRB_TransformBatcherEnableBatch for the same connections and keys
 * Each is run REPS times (the two batcher legs alternating) and the median is printed, as one JSON
 * line.  The two batcher legs must leave the same states (checked on every connection's read state). */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "brb_crypto.h"

#define KEY_BYTES 16

static double now_us(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e6 + t.tv_nsec * 1e-3;
}

static int cmp_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

static double median(double *v, int n)
{
    qsort(v, n, sizeof(*v), cmp_double);
    return n & 1 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

struct bf_job {
    BRB_BLOWFISH_CTX *ctx;
    unsigned char *keys;
    uint64_t lo, hi;
};

static void *bf_worker(void *p)
{
    struct bf_job *j = p;
    for (uint64_t i = j->lo; i < j->hi; i++)
        BRB_Blowfish_Init(&j->ctx[i], j->keys + i * KEY_BYTES, KEY_BYTES);
    return NULL;
}

static double bf_loop(BRB_BLOWFISH_CTX *ctx, unsigned char *keys, uint64_t n, int threads)
{
    pthread_t th[64];
    struct bf_job job[64];
    const double t0 = now_us();
    for (int t = 0; t < threads; t++) {
        job[t] = (struct bf_job){ctx, keys, n * t / threads, n * (t + 1) / threads};
        if (pthread_create(&th[t], NULL, bf_worker, &job[t]) != 0)
            exit(2);
    }
    for (int t = 0; t < threads; t++)
        pthread_join(th[t], NULL);
    return now_us() - t0;
}

int main(int argc, char **argv)
{
    if (argc != 6) {
        fprintf(stderr, "usage: %s N_RC4 N_BF N_CONN THREADS REPS\n", argv[0]);
        return 2;
    }
    const uint64_t n_rc4 = strtoull(argv[1], NULL, 10), n_bf = strtoull(argv[2], NULL, 10);
    const uint64_t n_conn = strtoull(argv[3], NULL, 10);
    const int threads = atoi(argv[4]), reps = atoi(argv[5]);
    if (threads < 1 || threads > 64 || reps < 1 || reps > 64 || !n_rc4 || !n_bf || !n_conn)
        return 2;
    const uint64_t n_max = n_rc4 > n_conn ? (n_rc4 > n_bf ? n_rc4 : n_bf) : (n_conn > n_bf ? n_conn : n_bf);
    unsigned char *keys = malloc(n_max * KEY_BYTES);
    uint64_t x = 0x5EED0008;
    for (uint64_t i = 0; i < n_max * KEY_BYTES; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        keys[i] = (unsigned char)(x >> 56);
    }
    double t[64];

    BRB_RC4_State *st = calloc(n_rc4, sizeof(*st));
    for (int r = 0; r < reps; r++) {
        const double t0 = now_us();
        for (uint64_t i = 0; i < n_rc4; i++)
            BRB_RC4_Init(&st[i], keys + i * KEY_BYTES, KEY_BYTES);
        t[r] = now_us() - t0;
    }
    const double rc4_us = median(t, reps);

    BRB_BLOWFISH_CTX *ctx = malloc(n_bf * sizeof(*ctx));
    for (int r = 0; r < reps; r++)
        t[r] = bf_loop(ctx, keys, n_bf, 1);
    const double bf1_us = median(t, reps);
    for (int r = 0; r < reps; r++)
        t[r] = bf_loop(ctx, keys, n_bf, threads);
    const double bft_us = median(t, reps);

    BRB_TransformBatcher *b1 = BRB_TransformBatcherCreate((uint32_t)n_conn, 1 << 20, BRB_CRYPTO_FUNC_RC4_MD5);
    BRB_TransformBatcher *b2 = BRB_TransformBatcherCreate((uint32_t)n_conn, 1 << 20, BRB_CRYPTO_FUNC_RC4_MD5);
    if (!b1 || !b2) {
        fprintf(stderr, "BRB_TransformBatcherCreate: %s\n", BRB_CryptoGPU_LastError());
        return 1;
    }
    uint32_t *conns = malloc(n_conn * sizeof(*conns)), *lens = malloc(n_conn * sizeof(*lens));
    uint64_t *offs = malloc(n_conn * sizeof(*offs));
    for (uint64_t i = 0; i < n_conn; i++) {
        conns[i] = (uint32_t)i;
        offs[i] = i * KEY_BYTES;
        lens[i] = KEY_BYTES;
    }
    double tb[64];
    for (int r = 0; r < reps; r++) {
        double t0 = now_us();
        for (uint64_t i = 0; i < n_conn; i++)
            if (BRB_TransformBatcherEnable(b1, (uint32_t)i, keys + i * KEY_BYTES, KEY_BYTES) != 1) {
                fprintf(stderr, "Enable: %s\n", BRB_CryptoGPU_LastError());
                return 1;
            }
        t[r] = now_us() - t0;
        t0 = now_us();
        if (BRB_TransformBatcherEnableBatch(b2, conns, n_conn, keys, offs, lens) != 1) {
            fprintf(stderr, "EnableBatch: %s\n", BRB_CryptoGPU_LastError());
            return 1;
        }
        tb[r] = now_us() - t0;
    }
    const double loop_us = median(t, reps), batch_us = median(tb, reps);
    int same = 1;
    for (uint64_t i = 0; i < n_conn; i++) {
        BRB_RC4_State a, c;
        if (BRB_TransformBatcherGetState(b1, (uint32_t)i, BRB_CRYPTO_OP_READ, &a) != 1 ||
            BRB_TransformBatcherGetState(b2, (uint32_t)i, BRB_CRYPTO_OP_WRITE, &c) != 1 || memcmp(&a, &c, sizeof(a)) != 0)
            same = 0;
    }
    BRB_TransformBatcherDestroy(b1);
    BRB_TransformBatcherDestroy(b2);
    printf("{\"rc4_init_loop_us\": %.1f, \"rc4_keys\": %llu, \"bf_init_loop_1t_us\": %.1f, \"bf_init_loop_mt_us\": %.1f, "
           "\"bf_keys\": %llu, \"threads\": %d, \"enable_loop_us\": %.1f, \"enable_batch_us\": %.1f, \"conns\": %llu, "
           "\"reps\": %d, \"batcher_states_equal\": %s}\n",
           rc4_us, (unsigned long long)n_rc4, bf1_us, bft_us, (unsigned long long)n_bf, threads, loop_us, batch_us,
           (unsigned long long)n_conn, reps, same ? "true" : "false");
    free(keys);
    free(st);
    free(ctx);
    free(conns);
    free(lens);
    free(offs);
    return same ? 0 : 1;
}
