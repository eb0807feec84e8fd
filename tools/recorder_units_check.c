/*
 * recorder_units_check.c — the recorder's unit entry outside Python, for a sanitizer build:
 *   gcc -std=c11 -g -fsanitize=address,undefined -Iinclude tools/recorder_units_check.c ffvvc_amd/host/recorder.c ffvvc_amd/host/levels_pack.c
 * Reads the flat dump tests/recorder_units_cases.py dump() writes (recorder_cases.py's dump, then the slice index per CTU, the
 * vvc355_rec_pu array and the motion store), records the picture twice through ONE recorder object with vvc355_rec_ctu_units (CTUs in
 * raster order, then in reverse: the second run reuses the first one's buffers) and prints a digest of each run: FNV-1a over what
 * tools/recorder_check.c hashes, then the unit lists of vvc355_rec_units and their totals (recorder_units_cases.digest()).
 * With `--time REPS` in front of the dump (an optimised build, tools/recorder_units_time.py) it prints per repetition, in seconds, the
 * CTU calls and vvc355_rec_end_picture of the picture through vvc355_rec_ctu and then through vvc355_rec_ctu_units.
 * Exit status: 0, 2 for a dump it cannot read, 3 when the recorder refuses the picture.
 */
#define _POSIX_C_SOURCE 199309L
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "vvc_mi355_rec.h"

/* vvc355_recon_order lives in the HIP library: the CTUs with commands in raster order stand in for it (the order is not hashed) */
int vvc355_recon_order(const vvc355_recon_ctu *ctus, int ncx, int ncy, int32_t *order)
{
    int n = 0;
    for (int rs = 0; rs < ncx * ncy; rs++)
        if (ctus[rs].n_cmd)
            order[n++] = rs;
    return n;
}

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = p;
    for (size_t i = 0; i < n; i++)
        h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

static void *read_array(FILE *f, size_t n, size_t elem)
{
    void *p = malloc(n * elem + 1);
    if (!p || fread(p, elem, n, f) != n) {
        fprintf(stderr, "recorder_units_check: short dump\n");
        exit(2);
    }
    return p;
}

static double now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv)
{
    const int reps = (argc == 4 && !strcmp(argv[1], "--time")) ? atoi(argv[2]) : 0;
    if (argc != 2 && reps < 1) {
        fprintf(stderr, "usage: recorder_units_check [--time REPS] DUMP\n");
        return 2;
    }
    FILE *f = fopen(argv[argc - 1], "rb");
    int32_t head[6];
    if (!f || fread(head, 4, 6, f) != 6 || head[0] != 0x35354352) {
        fprintf(stderr, "recorder_units_check: %s is no dump\n", argv[argc - 1]);
        return 2;
    }
    const int n_ctu = head[1], n_cu = head[2], n_tu = head[3], n_tb = head[4], n_lv = head[5];
    vvc355_rec_params *par = read_array(f, 1, sizeof(*par));
    int32_t *first = read_array(f, (size_t)n_ctu + 1, 4), *flags = read_array(f, (size_t)n_ctu, 4);
    vvc355_rec_cu *cus = read_array(f, (size_t)n_cu, sizeof(*cus));
    vvc355_rec_tu *tus = read_array(f, (size_t)n_tu, sizeof(*tus));
    vvc355_rec_tb *tbs = read_array(f, (size_t)n_tb, sizeof(*tbs));
    int32_t *levels = read_array(f, (size_t)n_lv, 4);
    int32_t *n_motion = read_array(f, 1, 4);
    int32_t *slice = read_array(f, (size_t)n_ctu, 4);
    vvc355_rec_pu *pus = read_array(f, (size_t)n_cu, sizeof(*pus));
    int32_t *motion = read_array(f, (size_t)*n_motion, 4);
    fclose(f);
    /* the dump holds indices where the PODs hold pointers */
    for (int i = 0; i < n_cu; i++) {
        cus[i].tus = tus + (uintptr_t)cus[i].tus;
        pus[i].motion = (uintptr_t)pus[i].motion == UINTPTR_MAX ? NULL : motion + (uintptr_t)pus[i].motion;
    }
    for (int i = 0; i < n_tu; i++)
        tus[i].tbs = tbs + (uintptr_t)tus[i].tbs;
    for (int i = 0; i < n_tb; i++)
        tbs[i].levels = (uintptr_t)tbs[i].levels == UINTPTR_MAX ? NULL : levels + (uintptr_t)tbs[i].levels;

    vvc355_recorder *rec = vvc355_rec_create();
    int ret = rec ? 0 : VVC355_REC_E_NOMEM;
    for (int rep = 0; rep < reps && !ret; rep++) {
        double t[2][2];
        for (int units = 0; units < 2 && !ret; units++) {
            vvc355_rec_result res;
            ret = vvc355_rec_begin_picture(rec, par);
            const double t0 = now();
            for (int rs = 0; rs < n_ctu && !ret; rs++)
                ret = units ? vvc355_rec_ctu_units(rec, rs, flags[rs], slice[rs], cus + first[rs], pus + first[rs], first[rs + 1] - first[rs])
                            : vvc355_rec_ctu(rec, rs, flags[rs], cus + first[rs], first[rs + 1] - first[rs]);
            const double t1 = now();
            if (!ret)
                ret = vvc355_rec_end_picture(rec, &res);
            t[units][0] = t1 - t0, t[units][1] = now() - t1;
        }
        if (!ret)
            printf("%.6f %.6f %.6f %.6f %d\n", t[0][0], t[0][1], t[1][0], t[1][1], n_cu);
    }
    for (int run = 0; run < 2 && !ret && !reps; run++) {
        vvc355_rec_result res;
        vvc355_rec_units_result u;
        ret = vvc355_rec_begin_picture(rec, par);
        for (int k = 0; k < n_ctu && !ret; k++) {
            const int rs = run ? n_ctu - 1 - k : k;
            ret = vvc355_rec_ctu_units(rec, rs, flags[rs], slice[rs], cus + first[rs], pus + first[rs], first[rs + 1] - first[rs]);
        }
        if (!ret)
            ret = vvc355_rec_end_picture(rec, &res);
        if (!ret)
            ret = vvc355_rec_units(rec, &u);
        if (ret)
            break;
        int32_t *arena = malloc(4 * (size_t)res.arena_len + 4);
        for (uint64_t i = 0; i < res.arena_len; i++)
            arena[i] = 0x7EADBEEF;
        ret = vvc355_rec_fill_arena(rec, arena);
        uint64_t h = 0xCBF29CE484222325ull;
        h = fnv(h, &res.n_levels, offsetof(vvc355_rec_result, late_keep) - offsetof(vvc355_rec_result, n_levels));
        h = fnv(h, res.cmds, sizeof(*res.cmds) * (size_t)res.n_cmds);
        h = fnv(h, res.ctus, sizeof(*res.ctus) * (size_t)res.n_ctus);
        h = fnv(h, res.intra, 16 * (size_t)res.n_intra);
        h = fnv(h, res.inter, 16 * (size_t)res.n_inter);
        h = fnv(h, res.ts, 16 * (size_t)res.n_ts);
        h = fnv(h, res.intra_lv, sizeof(vvc355_tb_levels) * (size_t)res.n_intra);
        h = fnv(h, res.inter_lv, sizeof(vvc355_tb_levels) * (size_t)res.n_inter);
        h = fnv(h, res.ts_lv, sizeof(vvc355_tb_levels) * (size_t)res.n_ts);
        h = fnv(h, res.levels, 2 * (size_t)res.n_levels);
        h = fnv(h, arena, 4 * (size_t)res.arena_len);
        h = fnv(h, u.cu, sizeof(*u.cu) * (size_t)u.n_cu);
        h = fnv(h, u.cu_qp, (size_t)u.n_cu);
        h = fnv(h, u.tu, sizeof(*u.tu) * (size_t)u.n_tu);
        h = fnv(h, u.tu_qp_c, 2 * (size_t)u.n_tu);
        h = fnv(h, u.ctu_first_cu, 4 * ((size_t)n_ctu + 1));
        h = fnv(h, u.ctu_first_tu, 4 * ((size_t)n_ctu + 1));
        h = fnv(h, u.mvf, sizeof(*u.mvf) * (size_t)u.n_mvf);
        h = fnv(h, u.ctu_first_mvf, 4 * ((size_t)n_ctu + 1));
        h = fnv(h, u.inter, sizeof(*u.inter) * (size_t)u.n_inter);
        h = fnv(h, u.affine, sizeof(*u.affine) * (size_t)u.n_affine);
        h = fnv(h, u.gpm, sizeof(*u.gpm) * (size_t)u.n_gpm);
        h = fnv(h, u.ciip, sizeof(*u.ciip) * (size_t)u.n_ciip);
        h = fnv(h, &u.n_inter_jobs, 5 * sizeof(int32_t));
        printf("%016" PRIx64 "\n", h);
        free(arena);
    }
    vvc355_rec_destroy(rec);
    free(par); free(first); free(flags); free(cus); free(tus); free(tbs); free(levels); free(n_motion); free(slice); free(pus); free(motion);
    if (ret)
        fprintf(stderr, "recorder_units_check: refused with %d\n", ret);
    return ret ? 3 : 0;
}
