/* host_runner.c -- the file runners: reader -> engine threads -> writer (hpgv_run_assoc / tdt / aggregate / stats / vcf2epi /
 * filter / split / genome / grm / logistic / linear / cmh).  The VCF tools' own batch steps and writers are in host_vcftools.c, what a run keeps beside its result file in
 * host_sideout.c.
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"
#include <errno.h>

/* ---- the runners' pipeline: reader -> engine threads -> writer, batches in rotation ------------------ */
/* batches in rotation and engine threads: two engine threads per device (one batch's bus copies beside the other's
 * kernels) and three more batches than engines (reader ahead, writer behind); one device: 5 batches, 2 engines */
enum { B_FREE = 0, B_FILLED = 1, B_BUSY = 2, B_DONE = 3 };
typedef struct {
    pthread_mutex_t mu; pthread_cond_t cv;
    run_batch_t bt[RUN_NB_MAX]; int state[RUN_NB_MAX]; long seq[RUN_NB_MAX];
    int nb, n_engines;
    long n_filled, n_taken, n_written;                  /* sequence numbers handed out so far per stage */
    int eof, rc;
    run_t *run;
    size_t batch_bytes;
    line_reader_t *rd;
    double t_read, t_engine, t_write;
    char err[256];
} run_pipe_t;

static void pipe_fail(run_pipe_t *P, int rc, const char *msg) {      /* mu held */
    if (!P->rc) { P->rc = rc; snprintf(P->err, sizeof P->err, "%s", msg); }
    pthread_cond_broadcast(&P->cv);
}

static void *pipe_reader(void *v) {
    run_pipe_t *P = (run_pipe_t *)v;
    for (;;) {
        pthread_mutex_lock(&P->mu);
        int k = -1;
        while (!P->rc) {
            for (int i = 0; i < P->nb && k < 0; i++) if (P->state[i] == B_FREE) k = i;
            if (k >= 0) break;
            pthread_cond_wait(&P->cv, &P->mu);
        }
        if (P->rc) { pthread_mutex_unlock(&P->mu); return NULL; }
        P->state[k] = B_BUSY;
        pthread_mutex_unlock(&P->mu);
        const double t0 = now_s();
        if (!P->bt[k].text) P->bt[k].text = text_buf_get(P->bt[k].text_cap);
        const size_t n = !P->bt[k].text ? (size_t)-1 : P->rd->devwin ? read_lines_dev(P->rd, P->bt[k].text, P->bt[k].text_cap, P->batch_bytes) : read_lines(P->rd, P->bt[k].text, P->batch_bytes);
        P->bt[k].dev_text = P->rd->last_dev; P->bt[k].dev_ctx = P->rd->devwin ? P->rd->last_ctx : NULL;
        P->bt[k].dev_base = P->rd->last_base; P->bt[k].dev_tiles = P->rd->last_dev ? P->rd->last_tiles : NULL; P->bt[k].dev_n_tiles = P->rd->last_n_tiles;
        const double dt = now_s() - t0;
        pthread_mutex_lock(&P->mu);
        P->t_read += dt;
        if (n == (size_t)-1) { P->state[k] = B_FREE; pipe_fail(P, HPGV_ERR_UNSUPPORTED, "read error, or a VCF line is longer than batch_bytes"); pthread_mutex_unlock(&P->mu); return NULL; }
        if (n == 0) { P->state[k] = B_FREE; P->eof = 1; pthread_cond_broadcast(&P->cv); pthread_mutex_unlock(&P->mu); return NULL; }
        P->bt[k].bytes = n; P->seq[k] = P->n_filled++; P->state[k] = B_FILLED;
        pthread_cond_broadcast(&P->cv);
        pthread_mutex_unlock(&P->mu);
    }
}

/* the tool's engine call over a batch; *what: its name, for the failure message.  *again: the batch held more of something than
 * there was room for, which there now is -- the call is to be repeated */
static int engine_call(run_t *R, run_batch_t *b, const char **what, int *again) {
    const run_tool_t tool = R->tool;
    const int m = b->max_lines;
    int rc = HPGV_OK;
    switch (tool) {
    case RUN_AGGREGATE: case RUN_STATS: { *what = "hpgv_stats_text";
        memset(b->smiss, 0, sizeof(int32_t) * (size_t)b->n_smiss);
        memset(b->cerr, 0, sizeof(int32_t) * (size_t)b->n_cerr);
        /* the 256-bin tables of multi-allelic lines: room for 4 096 of them (4 MB), grown to what a batch really holds -- one
         * per possible line is 1 KB x max_lines, hundreds of MB per batch for a narrow cohort in 256 MB windows */
        if (!b->mtab) { b->multi_cap = m < 4096 ? m : 4096; b->mtab = (int32_t *)malloc(sizeof(int32_t) * 256 * (size_t)b->multi_cap); if (!b->mtab) return HPGV_ERR_NOMEM; }
        b->n_multi = b->multi_cap;
        const int mend = tool == RUN_STATS && b->n_cerr > 0;
        const size_t gm = (size_t)m * (size_t)b->n_groups;
        rc = hpgv_stats_text_groups(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, b->c8, b->hw, b->hw + m,
                                    tool == RUN_STATS ? b->smiss : NULL, b->midx, b->mtab, &b->n_multi, mend ? b->merr : NULL, mend ? b->cerr : NULL,
                                    b->n_groups ? b->gc8 : NULL, b->n_groups ? b->ghw : NULL, b->n_groups ? b->ghw + gm : NULL);
        if (!rc && b->n_lines <= b->max_lines && b->n_multi > b->multi_cap) {      /* more multi-allelic lines than tables: again, with room */
            free(b->mtab);
            b->multi_cap = b->n_multi + b->n_multi / 8 + 16;
            if (b->multi_cap > b->max_lines) b->multi_cap = b->max_lines;
            b->mtab = (int32_t *)malloc(sizeof(int32_t) * 256 * (size_t)b->multi_cap);
            if (!b->mtab) return HPGV_ERR_NOMEM;
            *again = 1;
        }
        return rc;
    }
    case RUN_FILTER: case RUN_SPLIT:                       /* then the lines partitioned on the device (pipe_engine) */
        *what = tool == RUN_FILTER ? "hpgv_filter_text / hpgv_text_partition" : "hpgv_filter_text / hpgv_text_multisplit";
        return hpgv_filter_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status);
    case RUN_VCF2EPI: *what = "hpgv_epi_dataset_text";
        return hpgv_epi_dataset_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, b->rows);
    case RUN_TDT: *what = "hpgv_tdt_text";
        return hpgv_tdt_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                             b->ints, b->ints + m, b->dbl, b->dbl + m, b->dbl + 2 * m);
    case RUN_TDT_PERM: *what = "hpgv_tdt_perm_text";
        return hpgv_tdt_perm_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                                  b->ints, b->ints + m, b->dbl, b->dbl + m, b->dbl + 2 * m, b->n_ge, b->bmax);
    case RUN_CHISQ: case RUN_FISHER:
        if (R->clump) {                                  /* the same call, which also leaves the batch's candidate rows (p <= p2) */
            *what = "hpgv_assoc_select_text";
            rc = hpgv_assoc_select_text(g_ctx, tool, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                                        b->ints, b->ints + m, b->ints + 2 * m, b->ints + 3 * m,
                                        b->dbl, tool == RUN_CHISQ ? b->dbl + m : NULL, b->dbl + 2 * m,
                                        R->clump->p2, b->sel, b->crows, (size_t)R->n_samples, b->crows_cap, &b->n_sel);
            if (!rc && b->n_lines <= b->max_lines && b->n_sel > b->crows_cap) {      /* more candidates than rows: again, with room */
                free(b->crows);
                b->crows_cap = b->n_sel + b->n_sel / 8 + 16;
                b->crows = (uint8_t *)malloc((size_t)b->crows_cap * (size_t)(R->n_samples > 0 ? R->n_samples : 1));
                if (!b->crows) { b->crows_cap = 0; return HPGV_ERR_NOMEM; }
                *again = 1;
            }
            return rc;
        }
        *what = "hpgv_assoc_text";
        return hpgv_assoc_text(g_ctx, tool, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                               b->ints, b->ints + m, b->ints + 2 * m, b->ints + 3 * m,
                               b->dbl, tool == RUN_CHISQ ? b->dbl + m : NULL, b->dbl + 2 * m);
    case RUN_CHISQ_PERM: *what = "hpgv_assoc_perm_text";
        return hpgv_assoc_perm_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                                    b->ints, b->ints + m, b->ints + 2 * m, b->ints + 3 * m,
                                    b->dbl, b->dbl + m, b->dbl + 2 * m, b->n_ge, b->bmax);
    case RUN_MODEL: case RUN_MODEL_PERM:
        if (run_cmh(R) && run_mperm(R)) { *what = "hpgv_assoc_cmh_perm_text";      /* ... with the permutation within strata of the same batch in one call */
            return hpgv_assoc_cmh_perm_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, (hpgv_cmh_result *)b->dbl, b->n_ge, b->bmax);
        }
        if (run_cmh(R)) { *what = "hpgv_assoc_cmh_text";      /* the stratified association: its records in the model tests' doubles */
            return hpgv_assoc_cmh_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, (hpgv_cmh_result *)b->dbl, NULL);
        }
        *what = "hpgv_assoc_model_text";
        return hpgv_assoc_model_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                                     b->ints, b->dbl, b->dbl + 5 * (size_t)m, tool == RUN_MODEL_PERM ? b->n_ge : NULL, tool == RUN_MODEL_PERM ? b->bmax : NULL);
    case RUN_LOGISTIC: *what = "hpgv_assoc_logistic_text";
        return hpgv_assoc_logistic_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status,
                                        HPGV_RUN_LOGISTIC_MAX_ITER, HPGV_RUN_LOGISTIC_TOL, (hpgv_logistic_result *)b->dbl, NULL);
    case RUN_LINEAR:
        if (run_mperm(R)) { *what = "hpgv_assoc_linear_perm_text";      /* the records and the permutation of the same batch in one call */
            return hpgv_assoc_linear_perm_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, (hpgv_linear_result *)b->dbl,
                                               b->t_obs, b->n_ge, b->bmax);
        }
        *what = "hpgv_assoc_linear_text";
        return hpgv_assoc_linear_text(g_ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, (hpgv_linear_result *)b->dbl, NULL);
    case RUN_GENOME: { *what = "hpgv_ibs_text";            /* on one device of the run, into that device's counts (a batch with more lines than room adds nothing) */
        hpgv_ibs_counts *d_counts = NULL;
        hpgv_ctx *ctx = run_genome_device(R, b, &d_counts);
        return hpgv_ibs_text(ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, b->ints, d_counts);
    }
    case RUN_GRM: { *what = "hpgv_grm_text";               /* the same dealing, into that device's pair sums */
        hpgv_ibs_counts *d_acc = NULL;
        hpgv_ctx *ctx = run_genome_device(R, b, &d_acc);
        if (R->score) {                                  /* a score run: the plan weighs the lines, the sums and the constants lie in one buffer */
            *what = "hpgv_score_text";
            const run_score_t *S = R->score;
            const size_t pitch = run_score_acc_pitch(R);
            int64_t *acc = (int64_t *)d_acc;
            return hpgv_score_text(ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, run_score_weigh, R->score, S->n_scores, S->frac_bits,
                                   S->impute, b->ints, acc, pitch, acc + ((size_t)S->n_scores + 2) * pitch);
        }
        return hpgv_grm_text(ctx, b->text, b->bytes, m, &b->n_lines, b->line_off, b->field_off, b->status, R->frac_bits, R->min_maf, b->ints, (hpgv_grm_acc *)d_acc);
    }
    }
    return rc;
}

static void *pipe_engine(void *v) {
    run_pipe_t *P = (run_pipe_t *)v;
    const run_tool_t tool = P->run->tool;
    for (;;) {
        pthread_mutex_lock(&P->mu);
        int k = -1;
        while (!P->rc) {
            for (int i = 0; i < P->nb && k < 0; i++) if (P->state[i] == B_FILLED && P->seq[i] == P->n_taken) k = i;
            if (k >= 0 || (P->eof && P->n_taken == P->n_filled)) break;
            pthread_cond_wait(&P->cv, &P->mu);
        }
        if (P->rc || k < 0) { pthread_mutex_unlock(&P->mu); return NULL; }
        P->state[k] = B_BUSY; P->n_taken++;
        pthread_mutex_unlock(&P->mu);
        const double t0 = now_s();
        run_batch_t *b = &P->bt[k];
        int rc = HPGV_OK; const char *what = "";                    /* what: the engine call, for the failure message */
        /* tokenize the device copy in place (on the device that holds it): no H2D of the text -- and, when the decoder left its tile
         * records, no counting sweep over it either */
        if (b->dev_text) (void)hpgv_text_alias_tiles(b->dev_ctx ? b->dev_ctx : g_ctx, b->text, b->dev_text, b->dev_base, b->dev_tiles, (uint64_t)b->dev_n_tiles);
        /* max_lines is sized for complete records; a batch of short (damaged) lines can hold more: the
         * engine reports the true count, the arrays grow and the batch is done again */
        for (int attempt = 0; attempt < 4; attempt++) {
            int again = 0;
            rc = engine_call(P->run, b, &what, &again);
            if (again) continue;
            if (rc || b->n_lines <= b->max_lines) break;
            free(b->mtab); b->mtab = NULL;
            if (run_batch_reserve(b, b->n_lines)) { rc = HPGV_ERR_NOMEM; break; }
        }
        if (tool == RUN_FILTER && !rc) rc = filter_partition(b);      /* before the alias is dropped: the window is the source */
        if (tool == RUN_SPLIT && !rc) rc = split_partition(b);
        if (b->dev_text) (void)hpgv_text_alias(b->dev_ctx ? b->dev_ctx : g_ctx, b->text, NULL);
        const double dt = now_s() - t0;
        pthread_mutex_lock(&P->mu);
        P->t_engine += dt;
        if (rc) {
            char msg[256];
            snprintf(msg, sizeof msg, "%s failed (%d): %s", what, rc, rc == HPGV_ERR_NOMEM ? "out of memory" : hpgv_last_error(g_ctx));
            pipe_fail(P, rc, msg);
            pthread_mutex_unlock(&P->mu);
            return NULL;
        }
        if (run_mperm(P->run)) {                          /* the batch's maxima into the run's: max is order-independent */
            double *tmax = P->run->PM->tmax;
            for (int q = 0; q < P->run->n_perms; q++) if (b->bmax[q] > tmax[q]) tmax[q] = b->bmax[q];
        }
        P->state[k] = B_DONE;
        pthread_cond_broadcast(&P->cv);
        pthread_mutex_unlock(&P->mu);
    }
}

/* ---- one run, stage by stage: input (in run_file), cohort, outputs, pipeline, finish ---------------------- */
/* the pedigree: the trios of the PED whose three members are VCF columns (every row with both parents named, whatever its
 * phenotype).  For stats, installed when there is one and their child columns kept; for the Mendelian filter, always */
static int set_trios(run_t *R, const sample_ids_t *ids, int for_stats) {
    const ped_table_t *ped = &R->ped;
    const size_t n = (size_t)ped->n + 1;
    int32_t *tf = (int32_t *)malloc(sizeof(int32_t) * n), *tm = (int32_t *)malloc(sizeof(int32_t) * n), *tc = (int32_t *)malloc(sizeof(int32_t) * n);
    uint8_t *ts = (uint8_t *)malloc(n);
    int nt = 0;
    for (int i = 0; i < ped->n; i++) {
        if (!strcmp(ped->pat[i], "0") || !strcmp(ped->mat[i], "0")) continue;
        const int cp = sample_ids_get(ids, ped->iid[i]), fp = sample_ids_get(ids, ped->pat[i]), mp = sample_ids_get(ids, ped->mat[i]);
        if (cp < 0 || fp < 0 || mp < 0) continue;
        tf[nt] = fp; tm[nt] = mp; tc[nt] = cp; ts[nt] = (uint8_t)ped->sex[i]; nt++;
    }
    int rc = HPGV_OK;
    if (nt > 0 || !for_stats) {
        if ((rc = hpgv_set_pedigree(g_ctx, R->n_samples, nt, tf, tm, tc, ts))) host_fail("hpgv_set_pedigree", rc);
        g_ped_key.set = 0;
    }
    free(tf); free(tm); free(ts);
    if (for_stats) { R->trio_child = tc; R->n_trios = nt; } else free(tc);
    return rc;
}

/* the condition of every VCF column by the PED's PHENO (a column without a PED row: HPGV_COND_OTHER), malloc'ed, or NULL without
 * memory; *matched: the PED rows that are columns */
static uint8_t *cohort_conditions(const run_t *R, const sample_ids_t *ids, int *matched) {
    uint8_t *cond = (uint8_t *)malloc((size_t)R->n_samples + 1);
    for (int j = 0; cond && j < R->n_samples; j++) cond[j] = HPGV_COND_OTHER;
    for (int i = 0; cond && i < R->ped.n; i++) { const int j = sample_ids_get(ids, R->ped.iid[i]); if (j >= 0) { cond[j] = (uint8_t)R->ped.pheno[i]; (*matched)++; } }
    return cond;
}

/* the assoc cohort of the case-control and trait stages on the device(s), from the condition vector as built so far; y: the trait,
 * or NULL.  With a covariate file (the regressions) a cohort sample without a line of finite values leaves the cohort first, and
 * the matched covariates follow the cohort; with a within file (run_cmh) a cohort sample without a line leaves it, and the strata
 * of those that stay -- numbered by first appearance in VCF column order -- follow the cohort; n_used: the samples that stayed */
static int assoc_cohort_install(run_t *R, uint8_t *cond, const double *y) {
    const int n_samples = R->n_samples;
    int rc = HPGV_OK;
    double *cov = NULL;
    if (R->covar) {
        uint8_t *have = (uint8_t *)malloc((size_t)n_samples + 1);
        cov = (double *)malloc(sizeof(double) * ((size_t)n_samples * (size_t)R->n_covar + 1));
        if (!have || !cov) rc = HPGV_ERR_NOMEM;
        if (!rc) rc = covar_table_match(R->covar, R->names, n_samples, R->n_covar, cov, (size_t)R->n_covar, have);
        for (int j = 0; !rc && j < n_samples; j++) if (!have[j]) cond[j] = HPGV_COND_OTHER;
        free(have);
    }
    int32_t *stratum = NULL;
    if (!rc && R->within) {
        uint8_t *take = (uint8_t *)malloc((size_t)n_samples + 1);
        stratum = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n_samples + 1));
        if (!take || !stratum) rc = HPGV_ERR_NOMEM;
        for (int j = 0; !rc && j < n_samples; j++) take[j] = cond[j] == HPGV_COND_AFFECTED || cond[j] == HPGV_COND_UNAFFECTED;
        if (!rc) rc = within_table_match(R->within, R->names, n_samples, take, stratum, &R->n_strata);
        for (int j = 0; !rc && j < n_samples; j++) if (stratum[j] < 0) cond[j] = HPGV_COND_OTHER;
        if (!rc && R->n_strata == 0) { snprintf(g_err, sizeof g_err, "no cohort sample has a line in the within file"); rc = HPGV_ERR_INVALID; }
        free(take);
    }
    for (int j = 0; !rc && j < n_samples; j++) R->n_used += cond[j] == HPGV_COND_AFFECTED || cond[j] == HPGV_COND_UNAFFECTED;
    if (!rc && (rc = hpgv_set_cohort(g_ctx, cond, n_samples))) host_fail("hpgv_set_cohort", rc);
    g_assoc_key.set = 0;
    if (!rc && cov && R->n_covar > 0 && (rc = hpgv_set_covariates(g_ctx, cov, n_samples, R->n_covar))) host_fail("hpgv_set_covariates", rc);
    if (!rc && y && (rc = hpgv_set_phenotype(g_ctx, y, n_samples))) host_fail("hpgv_set_phenotype", rc);
    if (!rc && stratum && (rc = hpgv_set_strata(g_ctx, stratum, n_samples, R->n_strata))) host_fail("hpgv_set_strata", rc);
    if (!rc && stratum && run_mperm(R)) {                 /* the run's label rows, once: shuffles within the strata of the cohort that stayed */
        uint8_t *labels = (uint8_t *)malloc((size_t)R->n_perms * (size_t)(n_samples > 0 ? n_samples : 1));
        if (!labels) rc = HPGV_ERR_NOMEM;
        if (!rc && (rc = hpgv_perm_labels_shuffle_within(cond, stratum, n_samples, R->n_perms, R->perm_seed, labels))) host_fail("hpgv_perm_labels_shuffle_within", rc);
        if (!rc && (rc = hpgv_set_perm_labels(g_ctx, labels, R->n_perms))) host_fail("hpgv_set_perm_labels", rc);
        free(labels);
    }
    free(cov); free(stratum);
    return rc;
}

/* the tool's cohort on the device(s), PED rows looked up by sample name (associate_samples_and_positions +
 * sort_individuals), then the device-side record filters */
static int run_cohort(run_t *R, const char *vcf_path, const char *ped_path) {
    const ped_table_t *ped = &R->ped;
    const int n_samples = R->n_samples;
    int rc = HPGV_OK;
    sample_ids_t *ids = sample_ids_new((size_t)n_samples);
    for (int j = 0; j < n_samples; j++) sample_ids_put(ids, R->names[j], j);
    const tool_traits_t *T = tool_of(R->tool);
    switch (T->cohort) {
    case COHORT_COLUMNS: {
        /* the engine scans the stats layout of all columns (get_variants_stats / get_sample_stats, hpgv_filter_text, hpgv_ibs_text, hpgv_grm_text); stats with a
         * PED: its phenotype groups, and its trios give the Mendelian errors (stats_runner.c:165-170,194-198) */
        rc = hpgv_set_stats_cohort(g_ctx, n_samples);
        g_stats_key.set = 0;
        if (rc) host_fail("hpgv_set_stats_cohort", rc);
        if (rc || R->tool != RUN_STATS || ped->n == 0) break;
        /* phenotype groups (stats_runner.c:47-50,165-170): the distinct values of the PED's PHENO column, numbered in
         * order of first appearance; a VCF column without a PED row belongs to no group */
        int32_t *group = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_samples + 1));
        R->group_names = (char **)malloc(sizeof(char *) * (size_t)(ped->n + 1));
        for (int j = 0; j < n_samples; j++) group[j] = -1;
        for (int i = 0; i < ped->n; i++) {
            int gidx = -1;
            for (int k = 0; k < R->n_groups; k++) if (!strcmp(R->group_names[k], ped->phe[i])) { gidx = k; break; }
            if (gidx < 0 && R->n_groups < 4096) { gidx = R->n_groups; R->group_names[R->n_groups++] = ped->phe[i]; }
            const int j = sample_ids_get(ids, ped->iid[i]);
            if (j >= 0) group[j] = gidx;
        }
        if (R->n_groups > 0) {
            rc = hpgv_set_stats_groups(g_ctx, group, n_samples, R->n_groups);
            g_group_key.set = 0;
            if (rc) host_fail("hpgv_set_stats_groups", rc);
        }
        free(group);
        if (!rc) rc = set_trios(R, ids, 1);
        break;
    }
    case COHORT_FAMILIES: {
        /* families in order of first appearance; father / mother = founders by sex (tdt.c:62-73);
         * counted children = rows with both parents named, affected, present in the VCF (tdt.c:139-148) */
        int32_t *fcol = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ped->n + 1)), *mcol = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ped->n + 1));
        int32_t *coff = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ped->n + 2)), *ccol = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ped->n + 1));
        uint8_t *csex = (uint8_t *)malloc((size_t)ped->n + 1);
        char *done = (char *)calloc((size_t)ped->n + 1, 1);
        int nf = 0, nc = 0;
        coff[0] = 0;
        for (int i = 0; i < ped->n; i++) {
            if (done[i]) continue;
            int father = -1, mother = -1;
            for (int k = i; k < ped->n; k++) {
                if (strcmp(ped->fid[k], ped->fid[i])) continue;
                done[k] = 1;
                if (!strcmp(ped->pat[k], "0") && !strcmp(ped->mat[k], "0") && !(father >= 0 && mother >= 0)) {
                    if (ped->sex[k] == HPGV_SEX_MALE) father = k; else if (ped->sex[k] == HPGV_SEX_FEMALE) mother = k;
                }
            }
            int fp = father >= 0 ? sample_ids_get(ids, ped->iid[father]) : -1, mp = mother >= 0 ? sample_ids_get(ids, ped->iid[mother]) : -1;
            fcol[nf] = (fp >= 0 && mp >= 0) ? fp : -1;
            mcol[nf] = (fp >= 0 && mp >= 0) ? mp : -1;
            if (fcol[nf] >= 0)
                for (int k = i; k < ped->n; k++) {
                    if (strcmp(ped->fid[k], ped->fid[i])) continue;
                    if (!strcmp(ped->pat[k], "0") || !strcmp(ped->mat[k], "0")) continue;       /* child->father && child->mother */
                    if (ped->pheno[k] != HPGV_COND_AFFECTED) continue;
                    int cp = sample_ids_get(ids, ped->iid[k]);
                    if (cp < 0) continue;
                    ccol[nc] = cp; csex[nc] = (uint8_t)ped->sex[k]; nc++;
                }
            coff[++nf] = nc;
        }
        rc = hpgv_set_families(g_ctx, n_samples, nf, fcol, mcol, coff, ccol, csex);
        g_tdt_key.set = 0;
        if (rc) host_fail("hpgv_set_families", rc);
        if (!rc && T->mperm) {                           /* the run's flip rows, once: a fair coin per family and permutation */
            uint8_t *flips = (uint8_t *)malloc((size_t)R->n_perms * (size_t)(nf > 0 ? nf : 1));
            if (!flips) rc = HPGV_ERR_NOMEM;
            if (!rc && (rc = hpgv_perm_flips_shuffle(nf, R->n_perms, R->perm_seed, flips))) host_fail("hpgv_perm_flips_shuffle", rc);
            if (!rc && (rc = hpgv_set_tdt_flips(g_ctx, flips, R->n_perms))) host_fail("hpgv_set_tdt_flips", rc);
            free(flips);
        }
        free(fcol); free(mcol); free(coff); free(ccol); free(csex); free(done);
        break;
    }
    case COHORT_CASE_CONTROL: {
        int matched = 0;
        uint8_t *cond = cohort_conditions(R, ids, &matched);
        if (!cond) { rc = HPGV_ERR_NOMEM; break; }
        if (matched == 0 && n_samples > 0) {             /* assert(individual) of assoc.c:92: a VCF whose samples the PED does not know */
            snprintf(g_err, sizeof g_err, "no sample of %s is a row of %s", vcf_path, ped_path);
            rc = HPGV_ERR_INVALID;
        }
        if (R->tool == RUN_VCF2EPI) {                                 /* get_individual_phenotypes, dataset_creator.c:279-300: affected, or not */
            for (int j = 0; j < n_samples; j++) {
                if (cond[j] != HPGV_COND_AFFECTED) cond[j] = HPGV_COND_UNAFFECTED;
                if (cond[j] == HPGV_COND_AFFECTED) R->epi_aff++; else R->epi_unaff++;
            }
        }
        if (!rc) rc = assoc_cohort_install(R, cond, NULL);
        if (!rc && T->mperm) {                                        /* the run's label rows, once: shuffles of the PED's conditions */
            uint8_t *labels = (uint8_t *)malloc((size_t)R->n_perms * (size_t)(n_samples > 0 ? n_samples : 1));
            if (!labels) rc = HPGV_ERR_NOMEM;
            if (!rc && (rc = hpgv_perm_labels_shuffle(cond, n_samples, R->n_perms, R->perm_seed, labels))) host_fail("hpgv_perm_labels_shuffle", rc);
            if (!rc && (rc = hpgv_set_perm_labels(g_ctx, labels, R->n_perms))) host_fail("hpgv_set_perm_labels", rc);
            free(labels);
        }
        free(cond);
        if (!rc && R->tool == RUN_FISHER) {
            double *lf = init_logarithm_array(n_samples * 10 > 16 ? n_samples * 10 : 16);     /* assoc_runner.c:164-166 */
            rc = hpgv_set_logfact(g_ctx, lf, (size_t)(n_samples * 10 > 16 ? n_samples * 10 : 16));
            g_lf_key.table = NULL;
            if (rc) host_fail("hpgv_set_logfact", rc);
            free(lf);
        }
        break;
    }
    case COHORT_TRAIT: {                                  /* the cohort: every sample with a trait and, with covariates, a line of finite ones */
        uint8_t *cond = (uint8_t *)malloc((size_t)n_samples + 1), *have = (uint8_t *)malloc((size_t)n_samples + 1);
        double *y = (double *)calloc((size_t)n_samples + 1, sizeof(double));
        if (!cond || !have || !y) rc = HPGV_ERR_NOMEM;
        for (int j = 0; !rc && j < n_samples; j++) cond[j] = HPGV_COND_OTHER;
        if (!rc && R->pheno) {                            /* the phenotype file's first value column */
            rc = covar_table_match(R->pheno, R->names, n_samples, 1, y, 1, have);
            for (int j = 0; !rc && j < n_samples; j++) if (have[j]) cond[j] = HPGV_COND_UNAFFECTED;
        } else if (!rc) {                                 /* the PED's sixth column as a number: not finite, or -9, is missing */
            for (int i = 0; i < ped->n; i++) {
                const int j = sample_ids_get(ids, ped->iid[i]);
                if (j < 0) continue;
                char *end;
                const double v = strtod(ped->phe[i], &end);
                if (end == ped->phe[i] || *end != 0 || !isfinite(v) || v == -9.0) continue;
                cond[j] = HPGV_COND_UNAFFECTED; y[j] = v;
            }
        }
        if (!rc) rc = assoc_cohort_install(R, cond, y);
        if (!rc && run_mperm(R)) {                        /* the run's orders, once: shuffles of the cohort that stayed */
            int32_t *order = (int32_t *)malloc(sizeof(int32_t) * (size_t)R->n_perms * (size_t)(n_samples > 0 ? n_samples : 1));
            if (!order) rc = HPGV_ERR_NOMEM;
            if (!rc && (rc = hpgv_perm_order_shuffle(cond, n_samples, R->n_perms, R->perm_seed, order))) host_fail("hpgv_perm_order_shuffle", rc);
            if (!rc && (rc = hpgv_set_linear_perms(g_ctx, order, R->n_perms))) host_fail("hpgv_set_linear_perms", rc);
            free(order);
        }
        free(cond); free(have); free(y);
        break;
    }
    }
    /* device-side record filters: the count filters scan the stats layout of all columns, the Mendelian filter the trios */
    const hpgv_run_filters_t *f = &R->filters;
    if (!rc && (f->min_maf >= 0.0 || f->max_missing >= 0.0)) {
        rc = hpgv_set_stats_cohort(g_ctx, n_samples);
        g_stats_key.set = 0;
        if (rc) host_fail("hpgv_set_stats_cohort", rc);
    }
    if (!rc && f->max_mendel_errors >= 0) rc = set_trios(R, ids, 0);
    if (!rc) (void)hpgv_set_text_filters(g_ctx, f->min_maf, f->max_missing, (long)f->max_mendel_errors);
    /* --inh-dom / --inh-rec scan the assoc layout: the tools that have not installed it get it from the PED (PHENO 2
     * affected, 1 unaffected, as the assoc runner); vcf2epi and the regressions keep their own classes */
    if (!rc && rec_filters_inheritance(R->rf)) {
        if (!tool_installs_assoc_cohort(R->tool)) {
            int matched = 0;
            uint8_t *cond = cohort_conditions(R, ids, &matched);
            if (!cond) rc = HPGV_ERR_NOMEM;
            if (!rc && (rc = hpgv_set_cohort(g_ctx, cond, n_samples))) host_fail("hpgv_set_cohort", rc);
            g_assoc_key.set = 0;
            free(cond);
        }
        const hpgv_run_record_filters_t *rf = rec_filters_of(R->rf);
        if (!rc && (rc = hpgv_set_text_inheritance_filters(g_ctx, rf->min_dominant, rf->min_recessive))) host_fail("hpgv_set_text_inheritance_filters", rc);
    }
    sample_ids_free(ids);
    return rc;
}

/* <prefix><suffix> created for writing; *path keeps its name for the messages */
static int create_out(FILE **f, char **path, const char *prefix, const char *suffix) {
    if (!(*path = (char *)malloc(strlen(prefix) + strlen(suffix) + 1))) return HPGV_ERR_NOMEM;
    sprintf(*path, "%s%s", prefix, suffix);
    if (!(*f = fopen(*path, "wb"))) { snprintf(g_err, sizeof g_err, "cannot create %s", *path); return HPGV_ERR_INVALID; }
    setvbuf(*f, NULL, _IOFBF, 1u << 20);
    return HPGV_OK;
}

/* the tool's output files (split: its files as the records come).  The filter tool's .rejected is created empty without
 * save_rejected (filter_runner.c:63-68); stats: one file per phenotype (stats_runner.c:267-297), and its accumulator */
static int run_outputs(run_t *R, const char *out_path) {
    if ((R->clump && run_clump_new(R)) || (run_mperm(R) && run_perm_new(R))) return HPGV_ERR_NOMEM;
    if (tool_of(R->tool)->pairs) return run_genome_new(R);      /* (their files are written when the run ends: run_genome_write, run_grm_write) */
    const char *suffix = R->tool == RUN_STATS ? ".stats-variants" : R->tool == RUN_FILTER ? (R->out_bgzf ? ".filtered.gz" : ".filtered") : "";
    int rc = R->tool == RUN_SPLIT ? HPGV_OK : create_out(&R->out, &R->path, out_path, suffix);
    if (!rc && R->tool == RUN_FILTER) rc = create_out(&R->out_rej, &R->path_rej, out_path, R->out_bgzf ? ".rejected.gz" : ".rejected");
    if (rc || R->tool != RUN_STATS) return rc;
    if (R->n_groups > 0) {
        R->gfd = (FILE **)calloc((size_t)R->n_groups, sizeof(FILE *));
        char *gp = (char *)malloc(strlen(out_path) + 300);
        for (int k = 0; R->gfd && gp && k < R->n_groups && !rc; k++) {
            snprintf(gp, strlen(out_path) + 300, "%s.phenotype-%.200s.stats-variants", out_path, R->group_names[k]);
            if (!(R->gfd[k] = fopen(gp, "w"))) { snprintf(g_err, sizeof g_err, "cannot create %s", gp); rc = HPGV_ERR_INVALID; }
            else fprintf(R->gfd[k], "#CHROM\tPOS\tREF\tALT\tALLELES_COUNT\tALLELES_FREQ\tGENOTYPES_COUNT\tMISS_AL\tMISS_GT\tMAF\tHWE_CHI2\tHWE_P\n");
        }
        free(gp);
        if (!R->gfd) return HPGV_ERR_NOMEM;
    }
    return rc ? rc : run_stats_new(R);
}

/* the output files' headers, once the batches are allocated */
static int run_headers(run_t *R) {
    FILE *out = R->out;
    const tool_traits_t *T = tool_of(R->tool);
    if (T->header) {                                     /* the sorted results: the first line, which the order check starts from */
        if (T->file == RUN_TDT) tdt_write_output_header(out);
        else if (T->file == RUN_CHISQ || T->file == RUN_FISHER) assoc_write_output_header((enum ASSOC_task)T->file, out);      /* (the reference's writers) */
        else fprintf(out, "%s\n", run_header(R));
        order_track_keep(&R->ord, run_header(R), strlen(run_header(R)));
        return HPGV_OK;
    }
    switch (R->tool) {
    case RUN_VCF2EPI: {                                  /* room for the number of variants, then the class sizes (dataset_creator.c:186-193) */
        const uint32_t head[3] = {0, R->epi_aff, R->epi_unaff};
        return fwrite(head, sizeof(uint32_t), 3, out) != 3 ? HPGV_ERR_INVALID : HPGV_OK;
    }
    case RUN_AGGREGATE: {
        /* write_vcf_header_nosamples after add_aggregator_header (aggregate_runner.c:171-173,226-245): the file's meta lines,
         * the INFO entries of the added fields (texts: etc/hpg-variant/vcf-info-fields.conf), the delimiter line without FORMAT
         * and samples */
        const int bad = R->chrom_off && fwrite(R->hdr, 1, R->chrom_off, out) != R->chrom_off;
        const char *pre = R->overwrite ? "" : "HPG_", *by = R->overwrite ? "" : "Calculated by HPG Variant: ";
        fprintf(out, "##INFO=<ID=%sAC,Number=.,Type=Integer,Description=\"%sAllele count in genotypes, for each ALT allele, in the same order as listed\">\n", pre, by);
        fprintf(out, "##INFO=<ID=%sAF,Number=.,Type=Float,Description=\"%sAllele Frequency, for each ALT allele, in the same order as listed\">\n", pre, by);
        fprintf(out, "##INFO=<ID=%sAN,Number=1,Type=Integer,Description=\"%sTotal number of alleles in called genotypes\">\n", pre, by);
        fprintf(out, "##INFO=<ID=HPG_GTC,Number=.,Type=String,Description=\"Calculated by HPG Variant: Genotype counts, in pairs genotype:count\">\n");
        fprintf(out, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
        return bad ? HPGV_ERR_INVALID : HPGV_OK;
    }
    case RUN_STATS:
        fprintf(out, "#CHROM\tPOS\tREF\tALT\tNUM_ALLELES\tALLELES_COUNT\tALLELES_FREQ\tGENOTYPES_COUNT\tMISS_AL\tMISS_GT\tMAF\tMEND_ER\tHWE_CHI2\tHWE_P\n");
        return HPGV_OK;
    case RUN_FILTER: return write_filter_header(out, R) || (R->save_rejected && write_filter_header(R->out_rej, R)) ? HPGV_ERR_INVALID : HPGV_OK;
    default: break;                                      /* split: each file gets the input's header when it is created; genome, grm: no file yet */
    }
    return HPGV_OK;
}

/* the pipeline: one reader thread (with its team of pread / inflate threads), two engine threads per device (each call
 * is H2D, tokenize, scan, statistics, D2H on its own stream, so two in flight overlap the copies of one batch with the
 * kernels of the other) and this thread as the writer (with its team of formatters); batches are written in file order */
static int run_pipeline(run_t *R, size_t batch_bytes) {
    line_reader_t *rd = &R->rd;
    run_pipe_t *P = (run_pipe_t *)calloc(1, sizeof *P);
    out_buf_t *fmt = (out_buf_t *)calloc(RUN_FMT_BUFS, sizeof *fmt);
    int rc = P && fmt ? HPGV_OK : HPGV_ERR_NOMEM, have = 0;
    if (P) {
        int devs = hpgv_group_size(g_ctx);
        P->n_engines = 2 * (devs < 1 ? 1 : devs);
        /* windows of a text decoded on member 0's device stay there; a batch is then a chain of short kernels and two
         * small copies back, which four in flight overlap better than two (8 GB of text: 0.111 -> 0.100 s) */
        if (rd->src.d_text && !g_env.no_device_windows) P->n_engines = rd->src.mp && 2 * rd->src.mp->n > 4 ? 2 * rd->src.mp->n : 4;
        if (g_env.engine_threads > 0) P->n_engines = (int)g_env.engine_threads;      /* diagnosis: engine threads (batches in flight on the devices) */
        if (P->n_engines > RUN_ENGINES_MAX) P->n_engines = RUN_ENGINES_MAX;
        P->nb = P->n_engines + 3;
        R->n_engines = P->n_engines;
    }
    /* windows of a text that is on the device are not copied anywhere, so they need not be as small as the caller's batches:
     * about 64 of them per file, 256 MB at most, amortise what a batch costs whatever its size (three waits for the
     * device and 50 us of short kernels beside 100 us per 64 MB of tokenizing and scanning) */
    if (P && rd->src.d_text && !g_env.no_device_windows && !g_env.no_large_windows) {
        size_t w = rd->src.text_est / 64;
        if (w > ((size_t)256 << 20)) w = (size_t)256 << 20;
        if (w > batch_bytes) batch_bytes = w;
    }
    for (; !rc && have < P->nb; have++) rc = run_batch_alloc(&P->bt[have], R, out_batch_cap(R, batch_bytes), R->n_samples, R->n_trios, R->n_groups);
    if (rc == HPGV_ERR_NOMEM) snprintf(g_err, sizeof g_err, "out of memory for the batch buffers");
    if (!rc) rc = run_headers(R);
    if (!rc) {
        pthread_mutex_init(&P->mu, NULL); pthread_cond_init(&P->cv, NULL);
        P->run = R; P->batch_bytes = batch_bytes; P->rd = rd;
        io_pool_t rpool, wpool;
        pool_init(&rpool, R->io_threads); pool_init(&wpool, R->io_threads);
        rd->src.pool = &rpool;
        if (rd->src.d_text && !g_env.no_device_windows) {      /* bgzip decoded on the device: windows of the device text from the first data line on */
            rd->src.dev_pos -= rd->carry_len; rd->carry_len = 0; rd->devwin = 1;
        }
        const int n_fmt = R->io_threads < RUN_FMT_BUFS / 2 ? R->io_threads : RUN_FMT_BUFS / 2;      /* two sets of buffers: one is written while the other is filled */
        file_writer_t fw;
        memset(&fw, 0, sizeof fw);
        /* a thread of its own writes the formatted result lines (write_batch) */
        const int use_fw = tool_writer_thread(R->tool) && !g_env.no_writer_thread && file_writer_start(&fw, R->out);
        int fmt_set = 0;
        pthread_t th[1 + RUN_ENGINES_MAX];
        int n_th = 0;
        if (pthread_create(&th[n_th], NULL, pipe_reader, P) == 0) n_th++;
        for (int e = 0; e < P->n_engines; e++) if (pthread_create(&th[n_th], NULL, pipe_engine, P) == 0) n_th++;
        pthread_mutex_lock(&P->mu);
        if (n_th < 2) pipe_fail(P, HPGV_ERR_NOMEM, "cannot start the pipeline threads");
        for (;;) {
            int k = -1;
            while (!P->rc) {
                for (int i = 0; i < P->nb && k < 0; i++) if (P->state[i] == B_DONE && P->seq[i] == P->n_written) k = i;
                if (k >= 0 || (P->eof && P->n_written == P->n_filled)) break;
                pthread_cond_wait(&P->cv, &P->mu);
            }
            if (P->rc || k < 0) break;
            P->state[k] = B_BUSY;
            pthread_mutex_unlock(&P->mu);
            const double t0 = now_s();
            const run_batch_t *b = &P->bt[k];
            const char *bad = NULL;                      /* what went wrong */
            if (tool_of(R->tool)->lines) {               /* the batch's records to the tool's file, and what the run counts of them */
                if (write_batch(R->out, b, fmt + (fmt_set ? RUN_FMT_BUFS / 2 : 0), n_fmt, &wpool, &R->ord, use_fw ? &fw : NULL)) bad = "cannot write the result file";
                for (int i = 0; i < b->n_lines; i++) if (record_passes(b, i)) R->written++;
                if (R->PM && !bad && run_perm_add(R, b)) bad = "out of memory for the permutation results";
                if (R->CL && !bad && run_clump_add(R, b)) bad = "out of memory for the clumping candidates";
                if (R->RS && !bad) run_stats_add(R, b);      /* (and the group files' lines: by this thread) */
            } else switch (R->tool) {
            case RUN_FILTER:                             /* two fwrites (the batch's text is the partition now) */
                if (write_filter_batch(R->out, R->save_rejected ? R->out_rej : NULL, b)) bad = "cannot write the result file";
                R->written += b->n_pass; R->rejected += b->n_rej;
                break;
            case RUN_SPLIT:                              /* one fwrite per bucket */
                if (write_split_batch(R, b)) bad = g_err;          /* (what split_file said) */
                R->written += b->n_pass; R->skipped += b->n_skip;
                break;
            case RUN_GENOME: run_genome_add(R, b); break;       /* no line per record: the records' terms, in file order */
            case RUN_GRM: if (!R->score) run_grm_add(R, b); break;      /* no line per record: the used records are counted (a score run: on the device) */
            default: break;
            }
            fmt_set ^= use_fw;
            const double dt = now_s() - t0;
            pthread_mutex_lock(&P->mu);
            P->t_write += dt;
            if (bad) {
                char msg[200];
                snprintf(msg, sizeof msg, "%.199s", bad);
                pipe_fail(P, HPGV_ERR_INVALID, msg);
                break;
            }
            P->state[k] = B_FREE; P->n_written++;
            pthread_cond_broadcast(&P->cv);
        }
        pthread_mutex_unlock(&P->mu);
        if (use_fw && file_writer_stop(&fw)) { pthread_mutex_lock(&P->mu); pipe_fail(P, HPGV_ERR_INVALID, "cannot write the result file"); pthread_mutex_unlock(&P->mu); }
        for (int i = 0; i < n_th; i++) pthread_join(th[i], NULL);
        rd->src.pool = NULL;
        pool_destroy(&rpool); pool_destroy(&wpool);
        if (P->rc) { rc = P->rc; snprintf(g_err, sizeof g_err, "%s%s%s", g_input_err, g_input_err[0] ? "; " : "", P->err); }
        g_run_times[0] = P->t_read; g_run_times[1] = P->t_engine; g_run_times[2] = P->t_write; g_run_times[5] = (double)P->n_filled;
        pthread_mutex_destroy(&P->mu); pthread_cond_destroy(&P->cv);
    }
    for (int k = 0; P && k < have; k++) run_batch_free(&P->bt[k]);
    for (int k = 0; fmt && k < RUN_FMT_BUFS; k++) free(fmt[k].p);
    free(fmt); free(P);
    return rc;
}

/* the outputs completed and closed, and the tool's last steps; rc: the run's so far */
static int run_finish(run_t *R, int rc, const char *out_path) {
    const tool_traits_t *T = tool_of(R->tool);
    if (R->tool == RUN_VCF2EPI && R->out && !rc) {       /* finally the real number of variants (dataset_creator.c:208-212) */
        const uint32_t nv = (uint32_t)R->written;
        if (fseek(R->out, 0, SEEK_SET) != 0 || fwrite(&nv, sizeof nv, 1, R->out) != 1) { snprintf(g_err, sizeof g_err, "cannot write %s", out_path); rc = HPGV_ERR_INVALID; }
    }
    if (R->tool == RUN_FILTER && R->out_bgzf && ((R->out && bgzf_write_eof(R->out)) || (R->out_rej && bgzf_write_eof(R->out_rej))) && !rc) {      /* (.rejected.gz without save_rejected: a valid, empty bgzip file) */
        snprintf(g_err, sizeof g_err, "cannot write %s", out_path); rc = HPGV_ERR_INVALID;
    }
    if (R->out && fclose(R->out) != 0 && !rc) { snprintf(g_err, sizeof g_err, "cannot write %s", R->path); rc = HPGV_ERR_INVALID; }
    if (R->out_rej && fclose(R->out_rej) != 0 && !rc) { snprintf(g_err, sizeof g_err, "cannot write %s", R->path_rej); rc = HPGV_ERR_INVALID; }
    if (split_files_close(&R->SF, R->out_bgzf) && !rc) rc = HPGV_ERR_INVALID;
    for (int k = 0; R->gfd && k < R->n_groups; k++) if (R->gfd[k]) fclose(R->gfd[k]);
    if (T->sorts) {
        /* assoc_runner.c:255-261 (only a warning there); in order as written: nothing to do (HPGV_ALWAYS_SORT=1 reads the file
         * back and checks all the same) */
        const double t0 = now_s();
        const int sort = R->ord.disorder || !R->ord.have || g_env.always_sort;
        if (!rc && sort && hpgv_host_sort_output_file(out_path)) fprintf(stderr, "WARN: results could not be sorted by chromosome and position\n");
        else if (!rc && !sort && g_env.run_trace) fprintf(stderr, "hpgv run: the result file is in order as written\n");
        R->t_sort = now_s() - t0;
    }
    if (R->tool == RUN_STATS && !rc) rc = run_stats_write(R, out_path);
    if (run_mperm(R)) {
        if (!rc && R->PM) rc = run_perm_write(R, out_path);
        if (g_ctx) (void)(T->cohort == COHORT_FAMILIES ? hpgv_set_tdt_flips(g_ctx, NULL, 0) : T->cohort == COHORT_TRAIT ? hpgv_set_linear_perms(g_ctx, NULL, 0)
                                                                                                     : hpgv_set_perm_labels(g_ctx, NULL, 0));
        run_perm_free(R);
    }
    if (T->covar && g_ctx) (void)hpgv_set_covariates(g_ctx, NULL, 0, 0);
    if (run_cmh(R) && g_ctx) (void)hpgv_set_strata(g_ctx, NULL, 0, 0);
    if (T->cohort == COHORT_TRAIT && g_ctx) (void)hpgv_set_phenotype(g_ctx, NULL, 0);
    if (R->CL) {
        if (!rc) rc = run_clump_write(R, out_path);
        R->n_clumps = R->CL->n_clumps; R->n_truncated = R->CL->n_truncated;      /* for hpgv_run_assoc_clump, past the store */
        run_clump_free(R);
    }
    if (R->GN && R->tool == RUN_GRM) {
        if (!rc) rc = R->score ? run_score_write(R, out_path) : R->n_pcs ? run_pca_write(R, out_path) : run_grm_write(R, out_path);
    } else if (R->GN) {
        if (!rc) rc = run_genome_write(R, out_path);
        R->n_pairs = R->GN->n_pairs;                     /* for hpgv_run_genome, past the counts */
    }
    run_genome_free(R);
    run_stats_free(R);
    free(R->ord.last); free(R->gfd); free(R->group_names); free(R->path); free(R->path_rej); free(R->trio_child);
    const hpgv_run_filters_t *f = &R->filters;
    if (f->min_maf >= 0.0 || f->max_missing >= 0.0 || f->max_mendel_errors >= 0) (void)hpgv_set_text_filters(g_ctx, -1.0, -1.0, -1);
    if (rec_filters_inheritance(R->rf) && g_ctx) (void)hpgv_set_text_inheritance_filters(g_ctx, -1.0, -1.0);
    return rc;
}

static int run_file_held(run_t *R, const char *vcf_path, const char *ped_path, const char *out_path, size_t batch_bytes, long *n_variants_out);
/* the run holds the record filters of hpgv_run_set_record_filters as they are when it starts (stats, split, genome and grm: none) */
static int run_file(run_t *R, const char *vcf_path, const char *ped_path, const char *out_path, size_t batch_bytes, long *n_variants_out) {
    R->rf = tool_of(R->tool)->rec_filters ? rec_filters_take() : NULL;
    int rc = HPGV_OK;
    if (rec_filters_inheritance(R->rf) && !ped_path) {                /* filter_options_parsing.c:149-153 */
        snprintf(g_err, sizeof g_err, "the inheritance filters (--inh-dom / --inh-rec) need a PED file (ped_path is NULL)");
        rc = HPGV_ERR_INVALID;
    } else rc = run_file_held(R, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
    rec_filters_put(R->rf);
    R->rf = NULL;
    return rc;
}

static int run_file_held(run_t *R, const char *vcf_path, const char *ped_path, const char *out_path, size_t batch_bytes, long *n_variants_out) {
    host_env_read();                                               /* the environment: once per run (hpgv_host.h "Environment") */
    const double t_enter = now_s();
    g_write_split[0] = g_write_split[1] = 0;
    g_input_err[0] = 0;
    int rc = ensure_engine();
    if (rc) return rc;
    if (batch_bytes < (1u << 16)) batch_bytes = 1u << 16;
    const run_tool_t tool = R->tool; R->io_threads = default_io_threads();      /* the input: the PED (assoc, TDT, vcf2epi), the VCF's header */
    if (!ped_path && tool_of(tool)->needs_ped) { snprintf(g_err, sizeof g_err, "this runner needs a PED file (ped_path is NULL)"); return HPGV_ERR_INVALID; }
    if (ped_path && (rc = ped_table_read(ped_path, &R->ped))) return rc;
    if (source_open(&R->rd.src, vcf_path)) { ped_table_free(&R->ped); snprintf(g_err, sizeof g_err, "cannot open VCF file %s", vcf_path); return HPGV_ERR_INVALID; }
    R->t_opened = now_s();
    R->n_samples = vcf_header_read(&R->rd, &R->hdr, &R->names, &R->chrom_off);
    R->t_header = now_s();
    if (R->n_samples < 0) { source_close(&R->rd.src); free(R->rd.carry); free(R->rd.chrom_line); free(R->hdr); ped_table_free(&R->ped); snprintf(g_err, sizeof g_err, "%s%sno #CHROM header line in %s", g_input_err, g_input_err[0] ? "; " : "", vcf_path); return HPGV_ERR_INVALID; }
    /* the run keeps the cohort lock (exclusive) until its pipeline is done: the engine threads scan with the layouts installed
     * here, and an adapter or another runner with a different cohort waits instead of swapping them mid-file */
    pthread_rwlock_wrlock(&g_cohort_lock);
    rc = run_cohort(R, vcf_path, ped_path);
    if (!rc) rc = run_outputs(R, out_path);
    const double t_start = now_s();
    cpu_set_t saved_cpus;
    const int numa_bound = numa_bind_to_device(&saved_cpus);        /* before the buffers are allocated and the threads start */
    if (!rc) rc = run_pipeline(R, batch_bytes);
    rc = run_finish(R, rc, out_path);
    numa_unbind(&saved_cpus, numa_bound);
    g_run_times[3] = R->t_sort; g_run_times[4] = now_s() - t_start;
    if (g_env.run_trace)
        fprintf(stderr, "hpgv run: %ld records, %.0f batches, %d io threads: read %.3f s, engine %.3f s (%d threads), write %.3f s (stages overlap), sort %.3f s, total %.3f s\n",
                R->written, g_run_times[5], R->io_threads, g_run_times[0], g_run_times[1], R->n_engines, g_run_times[2], R->t_sort, g_run_times[4]);
    if (g_env.run_trace && R->tool == RUN_SPLIT)
        fprintf(stderr, "hpgv run: split keys %.4f s (host, summed over the engine threads)\n", (double)R->key_ns * 1e-9);
    const double t_done = now_s();
    source_close(&R->rd.src); free(R->rd.carry); free(R->rd.tailbuf); free(R->rd.chrom_line); free(R->hdr); free(R->names); ped_table_free(&R->ped);
    if (n_variants_out) *n_variants_out = R->written;
    pthread_rwlock_unlock(&g_cohort_lock);
    if (g_env.run_trace)
        fprintf(stderr, "hpgv run: before the pipeline: PED and open %.4f s, VCF header %.4f s, cohort and buffers %.4f s; after it: %.4f s; of the write stage: formatting %.4f s, writing %.4f s\n",
                R->t_opened - t_enter, R->t_header - R->t_opened, t_start - R->t_header, now_s() - t_done, g_write_split[0], g_write_split[1]);
    return rc;
}

/* the runners' reader on its own: copies `in_path` (plain, gzip or BGZF) to `out_path` in whole-line batches
 * of at most batch_bytes; what the runners feed to the engine, batch by batch */
int hpgv_host_copy_lines(const char *in_path, const char *out_path, size_t batch_bytes, int skip_vcf_header, long *n_batches) {
    host_env_read();
    line_reader_t rd;
    memset(&rd, 0, sizeof rd);
    if (batch_bytes < (1u << 16)) batch_bytes = 1u << 16;
    if (source_open(&rd.src, in_path)) { snprintf(g_err, sizeof g_err, "cannot open %s", in_path); return HPGV_ERR_INVALID; }
    FILE *out = fopen(out_path, "wb");
    char *buf = (char *)malloc(batch_bytes);
    int rc = (out && buf) ? HPGV_OK : HPGV_ERR_INVALID;
    long nb = 0;
    io_pool_t pool;
    pool_init(&pool, default_io_threads());
    rd.src.pool = &pool;
    if (!rc && skip_vcf_header) {
        char *hdr = NULL, **names = NULL;
        if (vcf_header_read(&rd, &hdr, &names, NULL) < 0) { snprintf(g_err, sizeof g_err, "no #CHROM header line in %s", in_path); rc = HPGV_ERR_INVALID; }
        free(hdr); free(names);
    }
    while (!rc) {
        size_t n = read_lines(&rd, buf, batch_bytes);
        if (n == 0) break;
        if (n == (size_t)-1) { snprintf(g_err, sizeof g_err, "read error, or a line longer than batch_bytes, in %s", in_path); rc = HPGV_ERR_UNSUPPORTED; break; }
        if (!rd.eof && buf[n - 1] != '\n') { rc = HPGV_ERR_UNSUPPORTED; break; }
        if (fwrite(buf, 1, n, out) != n) { rc = HPGV_ERR_INVALID; break; }
        nb++;
    }
    if (out) fclose(out);
    pool_destroy(&pool);
    free(buf); free(rd.carry); free(rd.chrom_line); source_close(&rd.src);
    if (n_batches) *n_batches = nb;
    return rc;
}

static const hpgv_run_filters_t filters_off = { -1.0, -1.0, -1, -1, -1.0 };
void hpgv_run_set_filters(const hpgv_run_filters_t *filters) { g_filters = filters ? *filters : filters_off; }

void hpgv_host_last_run_times(double *seconds6) { memcpy(seconds6, g_run_times, sizeof g_run_times); }
int hpgv_run_assoc(const char *vcf_path, const char *ped_path, const char *out_path, enum ASSOC_task task,
                   size_t batch_bytes, long *n_variants_out) {
    if (task != CHI_SQUARE && task != FISHER) { snprintf(g_err, sizeof g_err, "task must be CHI_SQUARE or FISHER"); return HPGV_ERR_INVALID; }
    return run_file(&(run_t){ .tool = (run_tool_t)task, .filters = g_filters }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}

/* how the runs that check their arguments open: the count zeroed, then none of the paths (or the options) NULL -- msg: the run's own wording */
static int run_args(long *n_variants_out, int all_given, const char *msg) {
    if (n_variants_out) *n_variants_out = 0;
    if (!all_given) snprintf(g_err, sizeof g_err, "%s", msg);
    return !all_given;
}

/* the chi-square run with max(T) label permutation: hpgv_run_assoc(..., CHI_SQUARE, ...)'s file and <out_path>.mperm */
int hpgv_run_assoc_perm(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                        size_t batch_bytes, long *n_variants_out) {
    if (run_args(n_variants_out, vcf_path && ped_path && out_path, "vcf_path, ped_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (n_perms < 1) { snprintf(g_err, sizeof g_err, "n_perms must be at least 1"); return HPGV_ERR_INVALID; }
    return run_file(&(run_t){ .tool = RUN_CHISQ_PERM, .filters = g_filters, .n_perms = n_perms, .perm_seed = seed }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}

/* the association run with LD clumping of its results: hpgv_run_assoc's file and <out_path>.clumped */
int hpgv_run_assoc_clump(const char *vcf_path, const char *ped_path, const char *out_path, enum ASSOC_task task,
                         const hpgv_run_clump_options_t *opt, size_t batch_bytes, long *n_variants_out,
                         long *n_clumps_out, long *n_truncated_out) {
    if (n_clumps_out) *n_clumps_out = 0;
    if (n_truncated_out) *n_truncated_out = 0;
    if (run_args(n_variants_out, vcf_path && ped_path && out_path && opt, "vcf_path, ped_path, out_path and the options must not be NULL")) return HPGV_ERR_INVALID;
    if (task != CHI_SQUARE && task != FISHER) { snprintf(g_err, sizeof g_err, "task must be CHI_SQUARE or FISHER"); return HPGV_ERR_INVALID; }
    if (!(opt->p1 > 0.0 && opt->p1 <= 1.0) || !(opt->p2 > 0.0 && opt->p2 <= 1.0) || !(opt->p1 <= opt->p2)) {      /* (a NaN fails every comparison) */
        snprintf(g_err, sizeof g_err, "clumping needs 0 < p1 <= p2 <= 1"); return HPGV_ERR_INVALID;
    }
    if (opt->min_r2 != opt->min_r2) { snprintf(g_err, sizeof g_err, "min_r2 is NaN"); return HPGV_ERR_INVALID; }
    if (opt->window < 1 || opt->window > HPGV_LD_MAX_WINDOW) { snprintf(g_err, sizeof g_err, "window %d: 1 .. %d candidates", opt->window, HPGV_LD_MAX_WINDOW); return HPGV_ERR_INVALID; }
    run_t R = { .tool = (run_tool_t)task, .filters = g_filters, .clump = opt };
    const int rc = run_file(&R, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
    if (n_clumps_out) *n_clumps_out = R.n_clumps;
    if (n_truncated_out) *n_truncated_out = R.n_truncated;
    return rc;
}

/* the model tests' run: one line of five chi-squares and p-values per variant and, with n_perms >= 1, <out_path>.mperm of the
 * trend statistic */
int hpgv_run_assoc_model(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                         size_t batch_bytes, long *n_variants_out) {
    if (run_args(n_variants_out, vcf_path && ped_path && out_path, "vcf_path, ped_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (n_perms < 0) { snprintf(g_err, sizeof g_err, "n_perms must not be negative"); return HPGV_ERR_INVALID; }
    return run_file(&(run_t){ .tool = n_perms ? RUN_MODEL_PERM : RUN_MODEL, .filters = g_filters, .n_perms = n_perms, .perm_seed = seed }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}

/* the regressions' run: n_covar checked, the phenotype file (linear; NULL: the PED's sixth column), then the covariate file (NULL: none),
 * read and checked before the engine starts; then RUN_MODEL's pipeline with the tool's own engine call */
static int run_regression(run_tool_t tool, const char *vcf_path, const char *ped_path, const char *pheno_path, const char *covar_path, int n_covar,
                          const char *out_path, int n_perms, uint64_t seed, size_t batch_bytes, long *n_variants_out, long *n_samples_used_out) {
    if (n_covar < 0 || (n_covar > 0 && !covar_path)) { snprintf(g_err, sizeof g_err, "n_covar %d: not negative, and 0 without a covariate file", n_covar); return HPGV_ERR_INVALID; }
    covar_table_t T, P;
    memset(&T, 0, sizeof T); memset(&P, 0, sizeof P);
    int use = 0, rc = HPGV_OK;
    if (pheno_path && !(rc = covar_table_read(pheno_path, &P)) && covar_table_columns(&P, 1) < 0) rc = HPGV_ERR_INVALID;
    if (!rc && covar_path && !(rc = covar_table_read(covar_path, &T)) && (use = covar_table_columns(&T, n_covar)) < 0) rc = HPGV_ERR_INVALID;
    if (!rc) {
        run_t R = { .tool = tool, .filters = g_filters, .covar = covar_path ? &T : NULL, .n_covar = use, .pheno = pheno_path ? &P : NULL, .n_perms = n_perms, .perm_seed = seed };
        rc = run_file(&R, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
        if (n_samples_used_out && !rc) *n_samples_used_out = R.n_used;
    }
    covar_table_free(&T); covar_table_free(&P);
    return rc;
}

int hpgv_run_assoc_logistic(const char *vcf_path, const char *ped_path, const char *covar_path, int n_covar, const char *out_path,
                            size_t batch_bytes, long *n_variants_out, long *n_samples_used_out) {
    if (n_samples_used_out) *n_samples_used_out = 0;
    if (run_args(n_variants_out, vcf_path && ped_path && out_path, "vcf_path, ped_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    return run_regression(RUN_LOGISTIC, vcf_path, ped_path, NULL, covar_path, n_covar, out_path, 0, 0, batch_bytes, n_variants_out, n_samples_used_out);
}

/* the stratified association's run: the within file read and checked before the engine starts, then RUN_MODEL's pipeline with the
 * tool's own engine call */
int hpgv_run_assoc_cmh(const char *vcf_path, const char *ped_path, const char *within_path, const char *out_path,
                       size_t batch_bytes, long *n_variants_out, long *n_samples_used_out, int *n_strata_out) {
    if (n_samples_used_out) *n_samples_used_out = 0;
    if (n_strata_out) *n_strata_out = 0;
    if (run_args(n_variants_out, vcf_path && ped_path && within_path && out_path, "vcf_path, ped_path, within_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    covar_table_t W;
    int rc = within_table_read(within_path, &W);
    if (rc) return rc;
    run_t R = { .tool = RUN_MODEL, .filters = g_filters, .within = &W };
    rc = run_file(&R, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
    if (n_samples_used_out && !rc) *n_samples_used_out = R.n_used;
    if (n_strata_out && !rc) *n_strata_out = R.n_strata;
    covar_table_free(&W);
    return rc;
}

/* the same run with max(T) label permutation within the strata: hpgv_run_assoc_cmh's file and <out_path>.mperm */
int hpgv_run_assoc_cmh_perm(const char *vcf_path, const char *ped_path, const char *within_path, const char *out_path, int n_perms, uint64_t seed,
                            size_t batch_bytes, long *n_variants_out, long *n_samples_used_out, int *n_strata_out) {
    if (n_samples_used_out) *n_samples_used_out = 0;
    if (n_strata_out) *n_strata_out = 0;
    if (run_args(n_variants_out, vcf_path && ped_path && within_path && out_path, "vcf_path, ped_path, within_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (n_perms < 1) { snprintf(g_err, sizeof g_err, "n_perms must be at least 1"); return HPGV_ERR_INVALID; }
    covar_table_t W;
    int rc = within_table_read(within_path, &W);
    if (rc) return rc;
    run_t R = { .tool = RUN_MODEL, .filters = g_filters, .within = &W, .n_perms = n_perms, .perm_seed = seed };
    rc = run_file(&R, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
    if (n_samples_used_out && !rc) *n_samples_used_out = R.n_used;
    if (n_strata_out && !rc) *n_strata_out = R.n_strata;
    covar_table_free(&W);
    return rc;
}

int hpgv_run_assoc_linear(const char *vcf_path, const char *ped_path, const char *pheno_path, const char *covar_path, int n_covar,
                          const char *out_path, size_t batch_bytes, long *n_variants_out, long *n_samples_used_out) {
    if (n_samples_used_out) *n_samples_used_out = 0;
    if (run_args(n_variants_out, vcf_path && out_path, "vcf_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (!ped_path && !pheno_path) { snprintf(g_err, sizeof g_err, "the trait needs a PED file or a phenotype file (ped_path and pheno_path are NULL)"); return HPGV_ERR_INVALID; }
    return run_regression(RUN_LINEAR, vcf_path, ped_path, pheno_path, covar_path, n_covar, out_path, 0, 0, batch_bytes, n_variants_out, n_samples_used_out);
}

/* the linear run with max(T) permutations of the reduced model's residuals: hpgv_run_assoc_linear's file and <out_path>.mperm */
int hpgv_run_assoc_linear_perm(const char *vcf_path, const char *ped_path, const char *pheno_path, const char *covar_path, int n_covar,
                               const char *out_path, int n_perms, uint64_t seed, size_t batch_bytes, long *n_variants_out, long *n_samples_used_out) {
    if (n_samples_used_out) *n_samples_used_out = 0;
    if (run_args(n_variants_out, vcf_path && out_path, "vcf_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (n_perms < 1) { snprintf(g_err, sizeof g_err, "n_perms must be at least 1"); return HPGV_ERR_INVALID; }
    if (!ped_path && !pheno_path) { snprintf(g_err, sizeof g_err, "the trait needs a PED file or a phenotype file (ped_path and pheno_path are NULL)"); return HPGV_ERR_INVALID; }
    return run_regression(RUN_LINEAR, vcf_path, ped_path, pheno_path, covar_path, n_covar, out_path, n_perms, seed, batch_bytes, n_variants_out, n_samples_used_out);
}

int hpgv_run_tdt(const char *vcf_path, const char *ped_path, const char *out_path, size_t batch_bytes, long *n_variants_out) {
    return run_file(&(run_t){ .tool = RUN_TDT, .filters = g_filters }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}

/* the TDT run with max(T) family flips: hpgv_run_tdt's file and <out_path>.mperm */
int hpgv_run_tdt_perm(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                      size_t batch_bytes, long *n_variants_out) {
    if (run_args(n_variants_out, vcf_path && ped_path && out_path, "vcf_path, ped_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (n_perms < 1) { snprintf(g_err, sizeof g_err, "n_perms must be at least 1"); return HPGV_ERR_INVALID; }
    return run_file(&(run_t){ .tool = RUN_TDT_PERM, .filters = g_filters, .n_perms = n_perms, .perm_seed = seed }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}

/* run_aggregate (src/vcf-tools/aggregate/aggregate_runner.c:23-222) */
int hpgv_run_aggregate(const char *vcf_path, const char *out_path, int overwrite, size_t batch_bytes, long *n_variants_out) {
    return run_file(&(run_t){ .tool = RUN_AGGREGATE, .filters = g_filters, .overwrite = overwrite ? 1 : 0 }, vcf_path, NULL, out_path, batch_bytes, n_variants_out);
}

/* run_stats (src/vcf-tools/stats/stats_runner.c:23-420) without the per-phenotype files and the database */
int hpgv_run_stats(const char *vcf_path, const char *ped_path, const char *out_prefix, size_t batch_bytes, long *n_variants_out) {
    /* the per-sample counters are sums over every data line of a batch, so the record filters are not applied here */
    return run_file(&(run_t){ .tool = RUN_STATS, .filters = filters_off }, vcf_path, ped_path, out_prefix, batch_bytes, n_variants_out);
}

/* sample relatedness (include/hpgv.h "IBS"; PLINK's --genome): the pairs of samples with PI_HAT >= min_pi_hat in one file.  As in
 * hpgv_run_stats the record filters are not applied: the counts are sums over every record of a batch */
int hpgv_run_genome(const char *vcf_path, const char *out_path, double min_pi_hat, size_t batch_bytes, long *n_variants_out, long *n_pairs_out) {
    if (n_pairs_out) *n_pairs_out = 0;
    if (run_args(n_variants_out, vcf_path && out_path, "vcf_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    if (min_pi_hat != min_pi_hat) { snprintf(g_err, sizeof g_err, "min_pi_hat is NaN"); return HPGV_ERR_INVALID; }
    run_t R = { .tool = RUN_GENOME, .filters = filters_off, .min_pi_hat = min_pi_hat };
    const int rc = run_file(&R, vcf_path, NULL, out_path, batch_bytes, n_variants_out);
    if (n_pairs_out) *n_pairs_out = R.n_pairs;
    return rc;
}

/* the genetic relationship matrix (include/hpgv.h "GRM"; GCTA's --make-grm-bin) of the VCF's samples at hpgv_grm_frac_bits(min_maf):
 * <out_prefix>.grm.bin, .grm.N.bin and .grm.id.  As in hpgv_run_genome neither filter setter is applied.  *n_variants_out: the
 * USED records */
int hpgv_run_grm(const char *vcf_path, const char *out_prefix, double min_maf, size_t batch_bytes, long *n_variants_out, long *n_samples_out) {
    if (n_samples_out) *n_samples_out = 0;
    if (run_args(n_variants_out, vcf_path && out_prefix, "vcf_path and out_prefix must not be NULL")) return HPGV_ERR_INVALID;
    const int frac_bits = hpgv_grm_frac_bits(min_maf);
    if (frac_bits < 0) { snprintf(g_err, sizeof g_err, "min_maf %g: above 0, at most 0.5 (and not below 2e-9)", min_maf); return HPGV_ERR_INVALID; }
    run_t R = { .tool = RUN_GRM, .filters = filters_off, .min_maf = min_maf, .frac_bits = frac_bits };
    const int rc = run_file(&R, vcf_path, NULL, out_prefix, batch_bytes, n_variants_out);
    if (n_samples_out && !rc) *n_samples_out = R.n_samples;
    return rc;
}

/* allele scoring (include/hpgv.h "Score"; PLINK's --score): the per-sample sums of the score file's weights over the records it names,
 * at out_path.  A RUN_GRM run with a score plan: the same dealing of batches to devices, hpgv_score_text in place of hpgv_grm_text,
 * the devices' integers added when the run ends.  Neither filter setter is applied */
int hpgv_run_score(const char *vcf_path, const char *score_path, const char *out_path, int impute, size_t batch_bytes,
                   long *n_variants_out, long *n_samples_out, long *n_unmatched_out) {
    if (n_samples_out) *n_samples_out = 0;
    if (n_unmatched_out) *n_unmatched_out = 0;
    if (run_args(n_variants_out, vcf_path && score_path && out_path, "vcf_path, score_path and out_path must not be NULL")) return HPGV_ERR_INVALID;
    run_score_t S;
    int rc = run_score_read(score_path, impute, &S);     /* before the engine starts: a bad file writes nothing */
    if (rc) return rc;
    run_t R = { .tool = RUN_GRM, .filters = filters_off, .score = &S };
    rc = run_file(&R, vcf_path, NULL, out_path, batch_bytes, n_variants_out);
    if (n_samples_out && !rc) *n_samples_out = R.n_samples;
    if (n_unmatched_out && !rc) *n_unmatched_out = S.n_unmatched;
    run_score_free(&S);
    return rc;
}

/* the principal components of that matrix (include/hpgv.h "PCA"): hpgv_run_grm's pass unchanged, then run_pca_write (host_pca.c)
 * in place of the three files -- or before them, with write_grm */
int hpgv_run_pca(const char *vcf_path, const char *out_prefix, double min_maf, int n_pcs, int write_grm, size_t batch_bytes,
                 long *n_variants_out, long *n_samples_out, int *n_iter_out) {
    if (n_samples_out) *n_samples_out = 0;
    if (n_iter_out) *n_iter_out = 0;
    if (run_args(n_variants_out, vcf_path && out_prefix, "vcf_path and out_prefix must not be NULL")) return HPGV_ERR_INVALID;
    const int frac_bits = hpgv_grm_frac_bits(min_maf);
    if (frac_bits < 0) { snprintf(g_err, sizeof g_err, "min_maf %g: above 0, at most 0.5 (and not below 2e-9)", min_maf); return HPGV_ERR_INVALID; }
    if (n_pcs < 1 || n_pcs > 24) { snprintf(g_err, sizeof g_err, "n_pcs %d: 1 .. 24", n_pcs); return HPGV_ERR_INVALID; }
    run_t R = { .tool = RUN_GRM, .filters = filters_off, .min_maf = min_maf, .frac_bits = frac_bits, .n_pcs = n_pcs, .write_grm = write_grm != 0 };
    const int rc = run_file(&R, vcf_path, NULL, out_prefix, batch_bytes, n_variants_out);
    if (n_samples_out && !rc) *n_samples_out = R.n_samples;
    if (n_iter_out && !rc) *n_iter_out = R.n_iter;
    return rc;
}

/* run_filter (src/vcf-tools/filter/filter_runner.c:23-260): the records of the VCF that pass the filters of
 * hpgv_run_set_filters, and those that do not, in two files; without a filter nothing is written (hpg_variant_utils.c:220-226) */
int hpgv_run_filter(const char *vcf_path, const char *ped_path, const char *out_prefix, int save_rejected, size_t batch_bytes,
                    long *n_passed_out, long *n_rejected_out) {
    if (n_passed_out) *n_passed_out = 0;
    if (n_rejected_out) *n_rejected_out = 0;
    run_t R = { .tool = RUN_FILTER, .filters = g_filters, .save_rejected = save_rejected ? 1 : 0, .out_bgzf = out_compression_now() == HPGV_OUT_BGZF };
    const hpgv_run_filters_t *F = &R.filters;
    if (!vcf_path || !out_prefix) { snprintf(g_err, sizeof g_err, "vcf_path and out_prefix must not be NULL"); return HPGV_ERR_INVALID; }
    rec_filters_t *rf = rec_filters_take();
    const int any_rec = rf != NULL;                       /* (a setting without an active filter is stored as none) */
    rec_filters_put(rf);
    if (F->min_maf < 0.0 && F->max_missing < 0.0 && F->max_mendel_errors < 0 && F->num_alleles < 0 && F->min_quality < 0.0 && !any_rec) {
        snprintf(g_err, sizeof g_err, "no filter is set (hpgv_run_set_filters, hpgv_run_set_record_filters): the filter tool writes nothing without one"); return HPGV_ERR_INVALID;
    }
    if (F->max_mendel_errors >= 0 && !ped_path) { snprintf(g_err, sizeof g_err, "the Mendelian error filter needs a PED file (ped_path is NULL)"); return HPGV_ERR_INVALID; }
    const int rc = run_file(&R, vcf_path, ped_path, out_prefix, batch_bytes, n_passed_out);
    if (n_rejected_out) *n_rejected_out = R.rejected;
    return rc;
}

/* run_split (src/vcf-tools/split/split_runner.c:23-190, split_options_parsing.c:114-140): every record of the VCF to
 * <out_dir>/<split name>_<base of the input>, the split name from its CHROM or from INFO's DP */
int hpgv_run_split(const char *vcf_path, const char *out_dir, int criterion, const long *intervals, int n_intervals,
                   size_t batch_bytes, long *n_records_out, long *n_files_out, long *n_skipped_out) {
    if (n_records_out) *n_records_out = 0;
    if (n_files_out) *n_files_out = 0;
    if (n_skipped_out) *n_skipped_out = 0;
    if (!vcf_path || !out_dir) { snprintf(g_err, sizeof g_err, "vcf_path and out_dir must not be NULL"); return HPGV_ERR_INVALID; }
    if (criterion != HPGV_SPLIT_CHROMOSOME && criterion != HPGV_SPLIT_COVERAGE) { snprintf(g_err, sizeof g_err, "unknown split criterion %d", criterion); return HPGV_ERR_INVALID; }
    if (criterion == HPGV_SPLIT_COVERAGE) {
        if (!intervals || n_intervals < 1) { snprintf(g_err, sizeof g_err, "the coverage criterion needs at least one interval"); return HPGV_ERR_INVALID; }
        for (int j = 1; j < n_intervals; j++)
            if (intervals[j] <= intervals[j - 1]) { snprintf(g_err, sizeof g_err, "the coverage intervals must be strictly increasing"); return HPGV_ERR_INVALID; }
    }
    run_t R = { .tool = RUN_SPLIT, .filters = filters_off, .criterion = criterion, .iv = intervals,      /* no record filters: every record to a file */
                .n_iv = criterion == HPGV_SPLIT_COVERAGE ? n_intervals : 0, .dir = out_dir, .out_bgzf = out_compression_now() == HPGV_OUT_BGZF };
    const char *slash = strrchr(vcf_path, '/');
    const char *base = slash ? slash + 1 : vcf_path;
    size_t bl = strlen(base);
    if (bl > 3 && !strcmp(base + bl - 3, ".gz")) bl -= 3;                   /* the files hold plain text, or get their own .gz (HPGV_OUT_BGZF) */
    else if (bl > 4 && !strcmp(base + bl - 4, ".bgz")) bl -= 4;
    if (bl >= sizeof R.base) { snprintf(g_err, sizeof g_err, "the input's file name is too long"); return HPGV_ERR_INVALID; }
    struct stat st;
    if (mkdir(out_dir, 0777) != 0 && !(errno == EEXIST && stat(out_dir, &st) == 0 && S_ISDIR(st.st_mode))) {     /* create_directory: one level */
        snprintf(g_err, sizeof g_err, "cannot create the output directory %s", out_dir); return HPGV_ERR_INVALID;
    }
    memcpy(R.base, base, bl); R.base[bl] = 0;
    const int rc = run_file(&R, vcf_path, NULL, out_dir, batch_bytes, n_records_out);
    if (n_files_out) *n_files_out = R.files;
    if (n_skipped_out) *n_skipped_out = R.skipped;
    return rc;
}

int hpgv_run_vcf2epi(const char *vcf_path, const char *ped_path, const char *out_path, size_t batch_bytes, long *n_variants_out) {
    return run_file(&(run_t){ .tool = RUN_VCF2EPI, .filters = g_filters }, vcf_path, ped_path, out_path, batch_bytes, n_variants_out);
}
