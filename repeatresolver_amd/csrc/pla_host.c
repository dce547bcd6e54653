/* pla_host.c -- host side of the locus anchorer (include/pla.h), plain C and usable without a GPU: the readers of the assembly
 * and of the loci, the placement of every locus from the hits of pla_search (the GPU part, pla_device.hip), the writers and the
 * drop-in's run. */
#define _POSIX_C_SOURCE 200809L
#include "pla.h"

#include <stdlib.h>
#include <string.h>

void pla_hits_free(pla_hits *h)
{
    if (!h) return;
    free(h->pattern); free(h->orientation); free(h->contig); free(h->boundary); free(h->lo); free(h->hi); free(h->distance);
    memset(h, 0, sizeof *h);
}

void pla_contigs_free(pla_contigs *c)
{
    if (!c) return;
    if (c->name) for (int j = 0; j < c->nc; j++) free(c->name[j]);
    free(c->name); free(c->off); free(c->bases);
    memset(c, 0, sizeof *c);
}

void pla_loci_free(pla_loci *l)
{
    if (!l) return;
    if (l->name) for (int i = 0; i < l->n; i++) free(l->name[i]);
    free(l->name); free(l->left_len); free(l->copy_len); free(l->right_len); free(l->off); free(l->seq);
    free(l->aoff); free(l->anchored); free(l->side);
    memset(l, 0, sizeof *l);
}

static int is_base(int ch)
{
    switch (ch) { case 'a': case 'c': case 'g': case 't': case 'A': case 'C': case 'G': case 'T': return 1; default: return 0; }
}

/* a FASTA as records {header line without '>', sequence bytes}: what both readers share.  keep_other: a sequence byte that is no
 * base is stored as 'n' (1) or is an error (0). */
typedef struct records {
    int n, cap;
    char **header;
    long long *off;               /* [n + 1] */
    char *bases;
    long long nbases, bcap;
} records;

static void records_free(records *r)
{
    if (r->header) for (int j = 0; j < r->n; j++) free(r->header[j]);
    free(r->header); free(r->off); free(r->bases);
    memset(r, 0, sizeof *r);
}

static int read_records(const char *path, int keep_other, records *r)
{
    memset(r, 0, sizeof *r);
    FILE *f = fopen(path, "r");
    if (!f) return PWR_ERR_IO;
    int rc = PWR_OK, ch;
    r->cap = 16; r->bcap = 1 << 16;
    r->header = calloc((size_t)r->cap, sizeof(char *)); r->off = malloc(sizeof(long long) * ((size_t)r->cap + 1)); r->bases = malloc((size_t)r->bcap);
    if (!r->header || !r->off || !r->bases) rc = PWR_ERR_NOMEM;
    if (rc == PWR_OK) r->off[0] = 0;
    int at_line_start = 1;
    while (rc == PWR_OK && (ch = fgetc(f)) != EOF) {
        if (ch == '>' && at_line_start) {                                           /* a header: the rest of the line */
            size_t len = 0, cap = 64;
            char *h = malloc(cap);
            if (!h) { rc = PWR_ERR_NOMEM; break; }
            while ((ch = fgetc(f)) != EOF && ch != '\n') {
                if (len + 2 > cap) { cap *= 2; char *nh = realloc(h, cap); if (!nh) { rc = PWR_ERR_NOMEM; break; } h = nh; }
                h[len++] = (char)ch;
            }
            if (rc != PWR_OK) { free(h); break; }
            while (len && h[len - 1] == '\r') len--;
            h[len] = 0;
            if (r->n == r->cap) {
                const int ncap = r->cap * 2;
                char **nh = realloc(r->header, sizeof(char *) * (size_t)ncap);
                if (nh) r->header = nh;
                long long *no = realloc(r->off, sizeof(long long) * ((size_t)ncap + 1));
                if (no) r->off = no;
                if (!nh || !no) { free(h); rc = PWR_ERR_NOMEM; break; }
                r->cap = ncap;
            }
            r->header[r->n++] = h;
            r->off[r->n] = r->nbases;
            at_line_start = 1;
            continue;
        }
        at_line_start = ch == '\n';
        if (ch == '\n' || ch == '\r' || ch == ' ' || ch == '\t') continue;
        if (r->n == 0) { rc = PWR_ERR_INPUT; break; }                               /* sequence before the first '>' */
        if (!is_base(ch)) { if (!keep_other) { rc = PWR_ERR_INPUT; break; } ch = 'n'; }
        if (r->nbases == r->bcap) {
            char *nb = realloc(r->bases, (size_t)r->bcap * 2);
            if (!nb) { rc = PWR_ERR_NOMEM; break; }
            r->bases = nb; r->bcap *= 2;
        }
        r->bases[r->nbases++] = (char)ch;
        r->off[r->n] = r->nbases;
    }
    fclose(f);
    if (rc != PWR_OK) records_free(r);
    return rc;
}

/* the first word of a header, malloc'ed */
static char *first_word(const char *h)
{
    size_t len = 0;
    while (h[len] && h[len] != ' ' && h[len] != '\t') len++;
    char *w = malloc(len + 1);
    if (!w) return NULL;
    memcpy(w, h, len);
    w[len] = 0;
    return w;
}

int pla_read_contigs(const char *path, pla_contigs *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!path) return PWR_ERR_ARG;
    records r;
    int rc = read_records(path, 1, &r);
    if (rc != PWR_OK) return rc;
    out->name = calloc((size_t)r.n + 1, sizeof(char *));
    if (!out->name) { records_free(&r); return PWR_ERR_NOMEM; }
    out->nc = r.n;
    for (int j = 0; j < r.n; j++) {
        out->name[j] = first_word(r.header[j]);
        if (!out->name[j]) { records_free(&r); pla_contigs_free(out); return PWR_ERR_NOMEM; }
    }
    out->off = r.off; out->bases = r.bases;                                          /* taken over */
    r.off = NULL; r.bases = NULL;
    records_free(&r);
    return PWR_OK;
}

/* the number behind `key` in a header: "left=" -> the number behind the ':' that follows the label; "copy=" -> the number itself */
static int header_field(const char *h, const char *key, int after_colon, int *value)
{
    const char *p = h;
    const size_t kl = strlen(key);
    for (;;) {
        p = strstr(p, key);
        if (!p) return 0;
        if (p == h || p[-1] == ' ' || p[-1] == '\t') break;
        p += kl;
    }
    p += kl;
    if (after_colon) {
        if (*p == '-') p++;
        while (*p >= '0' && *p <= '9') p++;
        if (*p != ':') return 0;
        p++;
    }
    if (*p < '0' || *p > '9') return 0;
    long long v = 0;
    while (*p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); if (v > 0x7fffffff) return 0; p++; }
    *value = (int)v;
    return 1;
}

int pla_read_loci(const char *path, pla_loci *out)
{
    if (!out) return PWR_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (!path) return PWR_ERR_ARG;
    records r;
    int rc = read_records(path, 0, &r);
    if (rc != PWR_OK) return rc;
    const size_t n = (size_t)r.n;
    out->name = calloc(n + 1, sizeof(char *));
    out->left_len = malloc(sizeof(int) * (n + 1)); out->copy_len = malloc(sizeof(int) * (n + 1)); out->right_len = malloc(sizeof(int) * (n + 1));
    out->aoff = malloc(sizeof(long long) * (2 * n + 1)); out->anchored = malloc((size_t)r.nbases + 1); out->side = malloc(sizeof(int) * (2 * n + 1));
    if (!out->name || !out->left_len || !out->copy_len || !out->right_len || !out->aoff || !out->anchored || !out->side) rc = PWR_ERR_NOMEM;
    if (rc == PWR_OK) {
        out->n = r.n;
        out->aoff[0] = 0;
    }
    for (int i = 0; rc == PWR_OK && i < r.n; i++) {
        int L = 0, C = 0, R = 0;
        if (!header_field(r.header[i], "left=", 1, &L) || !header_field(r.header[i], "copy=", 0, &C) ||
            !header_field(r.header[i], "right=", 1, &R) || (long long)L + C + R != r.off[i + 1] - r.off[i]) { rc = PWR_ERR_INPUT; break; }
        out->name[i] = first_word(r.header[i]);
        if (!out->name[i]) { rc = PWR_ERR_NOMEM; break; }
        out->left_len[i] = L; out->copy_len[i] = C; out->right_len[i] = R;
        const char *s = r.bases + r.off[i];
        char *a = out->anchored + out->aoff[2 * i];
        for (int x = 0; x < L; x++) a[x] = s[L - 1 - x];                             /* the left flank from the boundary outwards */
        out->aoff[2 * i + 1] = out->aoff[2 * i] + L;
        memcpy(a + L, s + L + C, (size_t)R);
        out->aoff[2 * i + 2] = out->aoff[2 * i + 1] + R;
        out->side[2 * i] = 0; out->side[2 * i + 1] = 1;
    }
    if (rc != PWR_OK) { records_free(&r); pla_loci_free(out); return rc; }
    out->off = r.off; out->seq = r.bases;
    r.off = NULL; r.bases = NULL;
    records_free(&r);
    return PWR_OK;
}

const char *pla_status_name(int status)
{
    static const char *const names[] = {"NONE", "AMBIGUOUS", "LEFT_ONLY", "RIGHT_ONLY", "PLACED", "BRIDGE", "INCONSISTENT", "CONFLICT"};
    return status >= 0 && status <= PLA_CONFLICT ? names[status] : "?";
}

int pla_place(int nloci, const int *left_pattern, const int *right_pattern, const pla_hits *hits, int max_span, pla_placement *out)
{
    if (nloci < 0 || max_span < 0 || !hits || hits->n < 0 || (nloci && (!left_pattern || !right_pattern || !out))) return PWR_ERR_ARG;
    if (hits->n && (!hits->pattern || !hits->orientation || !hits->contig || !hits->boundary || !hits->distance)) return PWR_ERR_ARG;
    for (int i = 0; i < nloci; i++) {
        pla_placement *p = &out[i];
        int at[2] = {-1, -1}, cnt[2] = {0, 0};
        const int pat[2] = {left_pattern[i], right_pattern[i]};
        for (int s = 0; s < 2; s++)
            for (int h = 0; pat[s] >= 0 && h < hits->n; h++)
                if (hits->pattern[h] == pat[s]) { if (!cnt[s]) at[s] = h; cnt[s]++; }
        memset(p, 0, sizeof *p);
        p->left_hits = cnt[0]; p->right_hits = cnt[1];
        p->left_contig = p->left_orientation = p->left_boundary = p->left_distance = -1;
        p->right_contig = p->right_orientation = p->right_boundary = p->right_distance = -1;
        p->lo = p->hi = -1;
        if (cnt[0] == 1) {
            const int h = at[0];
            p->left_contig = hits->contig[h]; p->left_orientation = hits->orientation[h]; p->left_boundary = hits->boundary[h]; p->left_distance = hits->distance[h];
        }
        if (cnt[1] == 1) {
            const int h = at[1];
            p->right_contig = hits->contig[h]; p->right_orientation = hits->orientation[h]; p->right_boundary = hits->boundary[h]; p->right_distance = hits->distance[h];
        }
        if (cnt[0] == 0 && cnt[1] == 0) p->status = PLA_NONE;
        else if (cnt[0] > 1 || cnt[1] > 1) p->status = PLA_AMBIGUOUS;
        else if (cnt[1] == 0) p->status = PLA_LEFT_ONLY;
        else if (cnt[0] == 0) p->status = PLA_RIGHT_ONLY;
        else if (p->left_contig != p->right_contig) p->status = PLA_BRIDGE;
        else {
            const int bl = p->left_boundary, br = p->right_boundary;
            p->lo = bl < br ? bl : br; p->hi = bl < br ? br : bl;
            p->status = PLA_INCONSISTENT;
            if (p->left_orientation == p->right_orientation) {
                p->has_span = 1;
                p->span = p->left_orientation ? bl - br : br - bl;
                if (p->span >= 0 && p->span <= max_span) p->status = PLA_PLACED;
            }
        }
    }
    /* two PLACED intervals of one contig that overlap: both are CONFLICT (decided on the statuses before any is changed) */
    char *hit = calloc((size_t)nloci + 1, 1);
    if (!hit) return PWR_ERR_NOMEM;
    for (int i = 0; i < nloci; i++) {
        if (out[i].status != PLA_PLACED) continue;
        for (int j = i + 1; j < nloci; j++)
            if (out[j].status == PLA_PLACED && out[j].left_contig == out[i].left_contig && out[i].lo < out[j].hi && out[j].lo < out[i].hi)
                hit[i] = hit[j] = 1;
    }
    for (int i = 0; i < nloci; i++) if (hit[i]) out[i].status = PLA_CONFLICT;
    free(hit);
    return PWR_OK;
}

static void put_int(FILE *f, int have, int v)
{
    if (have) fprintf(f, "\t%d", v); else fputs("\t-", f);
}

int pla_write_placements(const char *path, int nloci, const char *const *name, const pla_placement *p, const pla_contigs *contigs)
{
    if (!path || nloci < 0 || !contigs || (nloci && (!name || !p))) return PWR_ERR_ARG;
    for (int i = 0; i < nloci; i++)
        if (!name[i] || p[i].left_contig >= contigs->nc || p[i].right_contig >= contigs->nc) return PWR_ERR_ARG;
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    for (int i = 0; i < nloci; i++) {
        const pla_placement *q = &p[i];
        const int l = q->left_contig >= 0, r = q->right_contig >= 0;
        fprintf(f, "%s\t%s\t%s\t%s\t%s\t%s", name[i], pla_status_name(q->status), l ? contigs->name[q->left_contig] : "-",
                r ? contigs->name[q->right_contig] : "-", !l ? "-" : q->left_orientation ? "-" : "+", !r ? "-" : q->right_orientation ? "-" : "+");
        put_int(f, l, q->left_boundary); put_int(f, r, q->right_boundary);
        put_int(f, q->lo >= 0, q->lo); put_int(f, q->lo >= 0, q->hi); put_int(f, q->has_span, q->span);
        put_int(f, l, q->left_distance); put_int(f, r, q->right_distance);
        fputc('\n', f);
    }
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

static int complement(int ch)
{
    switch (ch) {
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    default: return ch;
    }
}

int pla_write_patched(const char *path, const pla_contigs *contigs, int nloci, const pla_placement *p, const char *copies,
                      const long long *coff)
{
    if (!path || !contigs || nloci < 0 || (nloci && (!p || !coff))) return PWR_ERR_ARG;
    for (int i = 0; i < nloci; i++) {
        if (coff[i + 1] < coff[i] || (coff[i + 1] > coff[i] && !copies)) return PWR_ERR_ARG;
        if (p[i].status != PLA_PLACED) continue;
        if (p[i].left_contig < 0 || p[i].left_contig >= contigs->nc || p[i].lo < 0 || p[i].hi < p[i].lo ||
            p[i].hi > contigs->off[p[i].left_contig + 1] - contigs->off[p[i].left_contig]) return PWR_ERR_ARG;
    }
    int *order = malloc(sizeof(int) * ((size_t)nloci + 1));
    if (!order) return PWR_ERR_NOMEM;
    FILE *f = fopen(path, "w");
    if (!f) { free(order); return PWR_ERR_IO; }
    for (int c = 0; c < contigs->nc; c++) {
        int k = 0;
        for (int i = 0; i < nloci; i++) {                                           /* this contig's intervals by (lo, hi, locus) */
            if (p[i].status != PLA_PLACED || p[i].left_contig != c) continue;
            int at = k++;
            while (at > 0 && (p[order[at - 1]].lo > p[i].lo || (p[order[at - 1]].lo == p[i].lo && p[order[at - 1]].hi > p[i].hi))) { order[at] = order[at - 1]; at--; }
            order[at] = i;
        }
        const char *s = contigs->bases + contigs->off[c];
        const long long len = contigs->off[c + 1] - contigs->off[c];
        fprintf(f, ">%s patched=%d\n", contigs->name[c], k);
        long long pos = 0;
        for (int a = 0; a < k; a++) {
            const pla_placement *q = &p[order[a]];
            const char *copy = copies + coff[order[a]];
            const long long cl = coff[order[a] + 1] - coff[order[a]];
            if (q->lo > pos) fwrite(s + pos, 1, (size_t)(q->lo - pos), f);
            if (q->left_orientation) for (long long x = cl - 1; x >= 0; x--) fputc(complement((unsigned char)copy[x]), f);
            else if (cl) fwrite(copy, 1, (size_t)cl, f);
            if (q->hi > pos) pos = q->hi;
        }
        if (len > pos) fwrite(s + pos, 1, (size_t)(len - pos), f);
        fputc('\n', f);
    }
    free(order);
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

static int write_anchors(const char *path, const pla_hits *h, const pla_loci *loci, const pla_contigs *contigs)
{
    FILE *f = fopen(path, "w");
    if (!f) return PWR_ERR_IO;
    for (int i = 0; i < h->n; i++)
        fprintf(f, "%s\t%s\t%c\t%s\t%d\t%d\t%d\t%d\n", loci->name[h->pattern[i] / 2], h->pattern[i] % 2 ? "right" : "left",
                h->orientation[i] ? '-' : '+', contigs->name[h->contig[i]], h->boundary[i], h->lo[i], h->hi[i], h->distance[i]);
    const int bad = ferror(f);
    if (fclose(f) != 0 || bad) return PWR_ERR_IO;
    return PWR_OK;
}

int pla_run_files(const char *loci_path, const char *assembly_path, int max_permille, int max_span, int reach, int min_len,
                  const char *prefix, int device, FILE *log)
{
    if (!loci_path || !assembly_path || !prefix || !log) return 1;
    pla_loci loci;
    pla_contigs contigs;
    pla_hits hits;
    pla_ctx *ctx = NULL;
    pla_placement *pl = NULL;
    int *lp = NULL;
    long long *coff = NULL;
    char *copies = NULL, *path = NULL;
    memset(&loci, 0, sizeof loci); memset(&contigs, 0, sizeof contigs); memset(&hits, 0, sizeof hits);
    int rc = max_span < 0 ? PWR_ERR_ARG : pla_read_loci(loci_path, &loci);
    if (rc == PWR_OK) rc = pla_read_contigs(assembly_path, &contigs);
    if (rc == PWR_OK) {
        const size_t n = (size_t)loci.n;
        fprintf(log, "loci %d, contigs %d, bases %lld\n", loci.n, contigs.nc, contigs.nc ? contigs.off[contigs.nc] : 0LL);
        pl = malloc(sizeof(pla_placement) * (n + 1)); lp = malloc(sizeof(int) * (2 * n + 2)); coff = malloc(sizeof(long long) * (n + 1));
        copies = malloc((size_t)(loci.n ? loci.off[loci.n] : 0) + 1); path = malloc(strlen(prefix) + 32);
        if (!pl || !lp || !coff || !copies || !path) rc = PWR_ERR_NOMEM;
    }
    if (rc == PWR_OK) {
        coff[0] = 0;
        for (int i = 0; i < loci.n; i++) {
            lp[i] = loci.left_len[i] ? 2 * i : -1; lp[loci.n + 1 + i] = loci.right_len[i] ? 2 * i + 1 : -1;
            memcpy(copies + coff[i], loci.seq + loci.off[i] + loci.left_len[i], (size_t)loci.copy_len[i]);
            coff[i + 1] = coff[i] + loci.copy_len[i];
        }
        rc = pla_create(&ctx, device);
    }
    if (rc == PWR_OK) rc = pla_open_text(ctx, contigs.nc, contigs.bases, contigs.off);
    if (rc == PWR_OK) rc = pla_search(ctx, 2 * loci.n, loci.anchored, loci.aoff, loci.side, reach, min_len, max_permille, &hits);
    if (rc == PWR_OK) rc = pla_place(loci.n, lp, lp + loci.n + 1, &hits, max_span, pl);
    if (rc == PWR_OK) { sprintf(path, "%s_Anchors", prefix); rc = write_anchors(path, &hits, &loci, &contigs); }
    if (rc == PWR_OK) { sprintf(path, "%s_Placements", prefix); rc = pla_write_placements(path, loci.n, (const char *const *)loci.name, pl, &contigs); }
    if (rc == PWR_OK) { sprintf(path, "%s_Patched.fasta", prefix); rc = pla_write_patched(path, &contigs, loci.n, pl, copies, coff); }
    if (rc == PWR_OK) {
        int by[PLA_CONFLICT + 1] = {0};
        unsigned long long cells = 0;
        double ms = 0.0;
        for (int i = 0; i < loci.n; i++) by[pl[i].status]++;
        pla_get_stats(ctx, &cells, &ms);
        fprintf(log, "hits %d\n", hits.n);
        for (int s = 0; s <= PLA_CONFLICT; s++) if (by[s]) fprintf(log, "%s %d\n", pla_status_name(s), by[s]);
        fprintf(log, "cells %llu, kernel %.3f ms\n", cells, ms);
        fprintf(log, "Files written: %s_Anchors %s_Placements %s_Patched.fasta\n", prefix, prefix, prefix);
    } else fprintf(log, "LocusAnchorer: %s\n", pwr_strerror(rc));
    pla_destroy(ctx);
    pla_hits_free(&hits); pla_loci_free(&loci); pla_contigs_free(&contigs);
    free(pl); free(lp); free(coff); free(copies); free(path);
    return rc == PWR_OK ? 0 : 1;
}
