/*
 * api.cpp -- the poporon C API of libpoporon_amd (include/poporon.h,
 * include/poporon/erasure.h, include/poporon/gf.h, include/poporon_amd.h).
 *
 * Host side of the drop-in boundary.  Object lifetimes and argument rules
 * follow the reference:
 *   config objects         src/poporon.c:214-233, :281-284, :301-304
 *   handle create/destroy  src/poporon.c:57-110, :172-212
 *   getters, version       src/poporon.c:306-373
 *   erasure list           src/erasure.c:12-127
 *   GF handle              src/gf.c:12-91
 *   generator polynomial   src/rs.c:29-82
 *   encode/decode checks   src/encode.c:236-252, src/decode.c:418-429, :596-612
 * All RS arithmetic on codewords runs in the HIP kernels (rs_kernels.hip);
 * there is no CPU codec in this library.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "poporon.h"
#include "poporon_amd.h"
#include "rs_device.h"
#include "rs_generic.h"
#include "bch_device.h"
#include "ldpc_device.h"
#include "ldpc_graph.h"
#include "cc_device.h"

#ifndef POPORON_BUILDTIME
#define POPORON_BUILDTIME 1
#endif
#define POPORON_VERSION_ID 20000000

#define EXPORT extern "C" __attribute__((visibility("default")))

/* ------------------------------------------------------------------------ */
/* error reporting                                                          */
/* ------------------------------------------------------------------------ */

static thread_local std::string g_last_error;

static bool fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static bool fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return false;
}

#define HIP_OK(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess)                                                                                         \
            return fail("%s failed: %s", #expr, hipGetErrorString(e_));                                               \
    } while (0)

EXPORT const char *poporon_amd_last_error(void) { return g_last_error.c_str(); }

/* ------------------------------------------------------------------------ */
/* objects                                                                  */
/* ------------------------------------------------------------------------ */

struct _poporon_erasure_t {
    uint32_t capacity;
    uint32_t erasure_count;
    uint32_t *erasure_positions;
    uint16_t *corrections; /* never written; kept for layout/ownership parity */
};

struct _poporon_gf_t {
    uint8_t symbol_size;
    uint8_t field_size; /* uint8 like the reference struct (src/internal/common.h:46-52) */
    uint16_t *log2exp;
    uint16_t *exp2log;
    uint16_t generator_polynomial;
};

struct poporon_rs_t {
    poporon_gf_t *gf;
    uint16_t first_consecutive_root;
    uint16_t primitive_element;
    uint16_t num_roots;
    uint16_t *generator_polynomial; /* log form */
};

struct _poporon_config_t {
    poporon_fec_type_t fec_type;
    uint8_t symbol_size;
    uint16_t generator_polynomial;
    uint16_t first_consecutive_root;
    uint16_t primitive_element;
    uint8_t num_roots;
    poporon_erasure_t *erasure;
    uint16_t *syndrome;
    uint8_t correction_capability; /* BCH */
    /* LDPC (src/internal/config.h; soft_llr is borrowed) */
    size_t block_size;
    uint32_t rate, matrix_type, column_weight;
    bool use_soft_decode, use_outer_interleave, use_inner_interleave;
    uint32_t interleave_depth, lifting_factor, max_iterations;
    const int8_t *soft_llr;
    size_t soft_llr_size;
    uint64_t seed;
};

#define NKERN 29
struct TimedLaunch {
    int kernel;
    hipEvent_t a, b;
};

/* a device buffer grown on demand (ensure_buf): cap counts the owner's units (codewords, list rows, bytes) */
struct DevBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
};

struct GpuCtx {
    bool timing = false;
    std::vector<TimedLaunch> pending;
    std::vector<hipEvent_t> event_pool;
    double total_ms[NKERN] = {};
    uint64_t launches[NKERN] = {};
    bool ready = false;
    int device = -1;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    RsDevTables *tab = nullptr; /* device (fast kernels) */
    RsGenTables *gtab = nullptr; /* device (general-parameter kernels) */
    uint8_t *rem = nullptr;     /* device workspace: rs_ws_bytes(rem_cap) (rs_device.h) */
    uint32_t *ltab = nullptr;   /* device (LDPC): the graph's tables, one allocation */
    uint8_t *lws = nullptr;     /* device (LDPC): messages of the decode kernel's workgroups, lws_bytes */
    size_t lws_bytes = 0;
    size_t rem_cap = 0;
    /* staging rows of the interleaved calls (rs_interleave.hip), RS_ILV_ROW
     * bytes per codeword; shared across streams under rem's ordering */
    DevBuf ilv;
    /* the rows before a decode, for the report calls (rs_report.hip): wire rows,
     * RS_ILV_ROW bytes per codeword allocated; ordered as ilv is */
    DevBuf rep;
    /* the plane calls' erasure lists (rs_planes.hip): plist.cap rows of plane_list_stride bytes, then plist.cap
     * counts; ordered as ilv is */
    DevBuf plist;
    /* the soft call's candidates (rs_soft.hip): soft.cap ok flags of the staged candidate rows, then soft.cap
     * corrected counts; ordered as ilv is */
    DevBuf soft;
    /* the wire form's device image (RS_ILV_WIRE_BYTES, rs_device.h); wire_ok: it
     * holds the handle's form as last set (ensure_wire) */
    uint8_t *wire = nullptr;
    size_t wire_cap = 0;
    bool wire_ok = false;
    /* Ordering of the workspace across streams: rem_done is recorded on the
     * stream of the last launch that read rem (rem_stream); a call on another
     * stream waits for it before overwriting rem. */
    hipEvent_t rem_done = nullptr;
    hipStream_t rem_stream = nullptr;
    bool rem_pending = false;
    /* single-codeword staging: device buffer + pinned host mirror, so that a
     * poporon_encode / poporon_decode call is one H2D copy, the kernels and
     * one D2H copy */
    uint8_t *stage = nullptr;
    uint8_t *hstage = nullptr;
    /* single-call paths without copies: ZC_BYTES of fine-grained (coherent,
     * GPU-uncached) host memory the kernels read and write directly (layout
     * ZC_* in rs_device.h); zc_dev is its device address, NULL if unavailable */
    uint8_t *zc = nullptr, *zc_dev = nullptr;
    uint32_t zc_seq = 0; /* completion words of the single-call kernels */
    /* the single-call server (rs_serve_k) on its own stream: srv_on while a
     * launch may still be serving, srv_id the id of the latest launch */
    hipStream_t sstream = nullptr;
    bool srv_on = false;
    uint32_t srv_id = 0;
    uint32_t srv_seq = 0; /* request words of the server (its own count: zc_seq also moves without it) */
    size_t stage_cap = 0;
    /* device registry (dev_register): batch_open while a batch call of this
     * handle is launching, then batch_ev (recorded behind its launches) until
     * the batch has run; other handles' servers stay off meanwhile */
    bool registered = false;
    bool batch_open = false;
    bool batch_ev_live = false;
    hipEvent_t batch_ev = nullptr;
    /* host-batch pipeline: PIPE_SLOTS chunks in flight, one stream each */
    struct PipeSlot {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        uint8_t *host = nullptr; /* pinned */
        uint8_t *dev = nullptr;
        size_t cap = 0;
        bool busy = false;
        size_t c0 = 0, n = 0; /* the chunk whose results the slot holds */
    } pipe[3];
    PipeSlot rslot; /* poporon_decode_batch_report's own slot */
};
#define PIPE_SLOTS 3

/* interleaved calls: codewords staged at a time (256 B each), default and the cap of the override */
#define ILV_CHUNK_DEFAULT ((size_t)1 << 20)
#define ILV_CHUNK_MAX (1ull << 24)
/* report calls: codewords snapshotted at a time (256 B each) */
#define REP_CHUNK_DEFAULT ((size_t)1 << 20)
#define REP_CHUNK_MAX (1ull << 24)

struct _poporon_t {
    poporon_fec_type_t fec_type;
    poporon_rs_t *rs;
    uint16_t primitive_inverse;
    poporon_erasure_t *erasure; /* borrowed, read live at every decode */
    uint16_t *ext_syndrome;     /* borrowed, read live at every decode */
    size_t last_corrected;
    bool supported; /* fast || generic */
    bool fast;      /* served by the RS(255,223) kernels (rs_kernels.hip, rs_correct.hip) */
    int decode_path; /* 0: by batch size, 1: split kernels (rs_fast.hip), 2: single kernel (rs_correct_k),
                      * 3: one codeword per wave (rs_wave_k) */
    int decode_tail; /* split kernels: 0 Forney and apply in one kernel (rs_forney_apply_k), 1 rs_forney_k then
                      * rs_apply_k, 2 the root search, Forney and apply in one kernel (rs_search_apply_k), 3 by
                      * the count: 2 where a workgroup of it has more than one batch, else 0 (split_tail);
                      * POPORON_AMD_DECODE_TAIL=fused|split|search, default: by the count where the batch size
                      * chooses the path, every stage its own kernel under POPORON_AMD_DECODE_PATH=split */
    bool generic;   /* served by the general-parameter kernels (rs_generic.hip) */
    bool lfsr_nr;   /* generic code, num_roots <= 32: batch encodes on the LFSR kernel (rsk_encode_nr) */
    bool nrsplit;   /* ... and large error-mode batches decode on the split kernels (params_nrsplit) */
    size_t ilv_chunk; /* codewords the interleaved calls stage at a time (POPORON_AMD_ILV_CHUNK) */
    size_t rep_chunk; /* codewords the report calls snapshot at a time (POPORON_AMD_REPORT_CHUNK) */
    int conv_path;    /* convolutional-interleaver layout kernels: RS_CONV_PATH_AUTO (the LDS tile where the window
                       * fits), _TILE or _DIRECT (POPORON_AMD_CONV_PATH=tile|direct) */
    /* wire form of the interleaved calls (poporon_amd_set_wire_form), the host copy: wf_set with a
     * map (wf_map; else the tables hold the identity), a sequence (wf_seq not empty) or both */
    bool wf_set, wf_map;
    uint8_t wf_code[256], wf_wire[256];
    std::vector<uint8_t> wf_seq;
    int gen_path;   /* general kernels: 0 by batch size, 1 one codeword per lane (rsg_*), 2 one per wave
                       (rsgw_*); POPORON_AMD_GENERIC=lane|wave */
    RsDevTables host_tab;
    RsCorrParams corr;
    RsGenTables gen_tab;
    RsGenParams gen;
    /* PPLN_FEC_BCH handles (rs == nullptr) */
    poporon_gf_t *bgf;
    BchParams bch;
    bool bch_ok; /* codewords fit 31 bits: served by bch.hip */
    /* PPLN_FEC_LDPC handles (rs == nullptr): the graph (owned), its device view, the decode settings */
    LdpcGraph *ldpc;
    LdpcDev ldev;
    int ldpc_path; /* 0: messages in LDS when they fit, 1: LDS, 2: global workspace (POPORON_AMD_LDPC_PATH) */
    uint32_t ldpc_max_iterations;
    bool ldpc_soft;
    const int8_t *ldpc_llr; /* borrowed, read at every poporon_decode */
    uint32_t ldpc_last_iterations;
    GpuCtx gpu;
};

/* ------------------------------------------------------------------------ */
/* GF(2^m) and generator (host setup)                                       */
/* ------------------------------------------------------------------------ */

static inline uint8_t gf_mod(const poporon_gf_t *gf, uint16_t v)
{
    while (v >= gf->field_size) {
        v = (uint16_t)(v - gf->field_size);
        v = (uint16_t)((v >> gf->symbol_size) + (v & gf->field_size));
    }
    return (uint8_t)v;
}

EXPORT void poporon_gf_destroy(poporon_gf_t *gf)
{
    if (!gf)
        return;
    free(gf->log2exp);
    free(gf->exp2log);
    free(gf);
}

EXPORT poporon_gf_t *poporon_gf_create(uint8_t symbol_size, uint16_t generator_polynomial)
{
    if (symbol_size < 1 || symbol_size > 16)
        return nullptr;
    poporon_gf_t *gf = (poporon_gf_t *)calloc(1, sizeof(poporon_gf_t));
    if (!gf)
        return nullptr;
    gf->symbol_size = symbol_size;
    gf->field_size = (uint8_t)((1u << symbol_size) - 1u);
    gf->generator_polynomial = generator_polynomial;
    gf->log2exp = (uint16_t *)calloc((size_t)gf->field_size + 1, sizeof(uint16_t));
    gf->exp2log = (uint16_t *)calloc((size_t)gf->field_size + 1, sizeof(uint16_t));
    if (!gf->log2exp || !gf->exp2log) {
        poporon_gf_destroy(gf);
        return nullptr;
    }
    /* powers of x reduced by the field polynomial; log(0) = field_size */
    gf->exp2log[0] = gf->field_size;
    gf->log2exp[gf->field_size] = 0;
    uint16_t x = 1;
    for (uint8_t i = 0; i < gf->field_size; i++) {
        gf->exp2log[x] = i;
        gf->log2exp[i] = x;
        x = (uint16_t)(x << 1);
        if (x & (1u << symbol_size))
            x ^= generator_polynomial;
        x &= gf->field_size;
    }
    if (x != gf->log2exp[0]) { /* not primitive: the walk did not close */
        poporon_gf_destroy(gf);
        return nullptr;
    }
    return gf;
}

EXPORT uint8_t poporon_gf_mod(poporon_gf_t *gf, uint16_t value) { return gf ? gf_mod(gf, value) : 0; }

EXPORT void poporon_rs_destroy(poporon_rs_t *rs)
{
    if (!rs)
        return;
    poporon_gf_destroy(rs->gf);
    free(rs->generator_polynomial);
    free(rs);
}

/* g(x) = prod_{i<num_roots} (x - alpha^(prim*(fcr+i))), stored in log form.
 * The root exponent is a uint16 accumulator as in the reference. */
EXPORT poporon_rs_t *poporon_rs_create(uint8_t symbol_size, uint16_t generator_polynomial,
                                       uint16_t first_consecutive_root, uint16_t primitive_element, uint8_t num_roots)
{
    poporon_gf_t *gf = poporon_gf_create(symbol_size, generator_polynomial);
    if (!gf)
        return nullptr;
    poporon_rs_t *rs = (poporon_rs_t *)calloc(1, sizeof(poporon_rs_t));
    if (!rs) {
        poporon_gf_destroy(gf);
        return nullptr;
    }
    rs->gf = gf;
    rs->first_consecutive_root = first_consecutive_root;
    rs->primitive_element = primitive_element;
    rs->num_roots = num_roots;
    rs->generator_polynomial = (uint16_t *)calloc((size_t)num_roots + 1, sizeof(uint16_t));
    if (!rs->generator_polynomial) {
        poporon_rs_destroy(rs);
        return nullptr;
    }
    uint16_t *g = rs->generator_polynomial;
    g[0] = 1;
    uint16_t root = (uint16_t)(first_consecutive_root * primitive_element);
    for (uint16_t i = 0; i < num_roots; i++, root = (uint16_t)(root + primitive_element)) {
        g[i + 1] = 1;
        for (uint16_t j = i; j > 0; j--)
            g[j] = g[j] ? (uint16_t)(g[j - 1] ^ gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[g[j]] + root))])
                        : g[j - 1];
        g[0] = gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[g[0]] + root))];
    }
    for (uint16_t i = 0; i <= num_roots; i++)
        g[i] = gf->exp2log[g[i]];
    return rs;
}

/* ------------------------------------------------------------------------ */
/* erasure list                                                             */
/* ------------------------------------------------------------------------ */

EXPORT void poporon_erasure_destroy(poporon_erasure_t *e)
{
    if (!e)
        return;
    free(e->erasure_positions);
    free(e->corrections);
    free(e);
}

EXPORT poporon_erasure_t *poporon_erasure_create(uint16_t num_roots, uint32_t initial_capacity)
{
    const uint32_t cap = initial_capacity > 0 ? initial_capacity : (uint32_t)num_roots;
    poporon_erasure_t *e = (poporon_erasure_t *)calloc(1, sizeof(poporon_erasure_t));
    if (!e)
        return nullptr;
    /* zero-filled (the reference leaves slots uninitialised; see quirk Q3) */
    e->erasure_positions = (uint32_t *)calloc(cap ? cap : 1, sizeof(uint32_t));
    e->corrections = (uint16_t *)calloc(cap ? cap : 1, sizeof(uint16_t));
    if (!e->erasure_positions || !e->corrections) {
        poporon_erasure_destroy(e);
        return nullptr;
    }
    e->capacity = cap;
    e->erasure_count = 0;
    return e;
}

EXPORT poporon_erasure_t *poporon_erasure_create_from_positions(uint16_t num_roots, const uint32_t *positions,
                                                                uint32_t count)
{
    if (!positions || count == 0)
        return nullptr;
    poporon_erasure_t *e = poporon_erasure_create(num_roots, count > num_roots ? count : num_roots);
    if (!e)
        return nullptr;
    memcpy(e->erasure_positions, positions, (size_t)count * sizeof(uint32_t));
    e->erasure_count = count;
    return e;
}

EXPORT bool poporon_erasure_add_position(poporon_erasure_t *e, uint32_t position)
{
    if (!e)
        return false;
    if (e->erasure_count >= e->capacity) {
        uint32_t cap = e->capacity * 2;
        if (cap < e->capacity + 32)
            cap = e->capacity + 32;
        uint32_t *np = (uint32_t *)realloc(e->erasure_positions, (size_t)cap * sizeof(uint32_t));
        if (!np)
            return false;
        e->erasure_positions = np;
        uint16_t *nc = (uint16_t *)realloc(e->corrections, (size_t)cap * sizeof(uint16_t));
        if (!nc)
            return false;
        e->corrections = nc;
        memset(e->erasure_positions + e->capacity, 0, (size_t)(cap - e->capacity) * sizeof(uint32_t));
        e->capacity = cap;
    }
    e->erasure_positions[e->erasure_count++] = position;
    return true;
}

EXPORT void poporon_erasure_reset(poporon_erasure_t *e)
{
    if (e)
        e->erasure_count = 0;
}

/* ------------------------------------------------------------------------ */
/* configs                                                                  */
/* ------------------------------------------------------------------------ */

EXPORT poporon_config_t *poporon_rs_config_create(uint8_t symbol_size, uint16_t generator_polynomial,
                                                  uint16_t first_consecutive_root, uint16_t primitive_element,
                                                  uint8_t num_roots, poporon_erasure_t *erasure, uint16_t *syndrome)
{
    poporon_config_t *c = (poporon_config_t *)calloc(1, sizeof(poporon_config_t));
    if (!c)
        return nullptr;
    c->fec_type = PPLN_FEC_RS;
    c->symbol_size = symbol_size;
    c->generator_polynomial = generator_polynomial;
    c->first_consecutive_root = first_consecutive_root;
    c->primitive_element = primitive_element;
    c->num_roots = num_roots;
    c->erasure = erasure;
    c->syndrome = syndrome;
    return c;
}

EXPORT poporon_config_t *poporon_config_rs_default(void)
{
    return poporon_rs_config_create(8, 0x11D, 1, 1, 32, nullptr, nullptr);
}

/* src/poporon.c:235-263: the 13 arguments are stored, soft_llr is borrowed */
EXPORT poporon_config_t *poporon_ldpc_config_create(size_t block_size, poporon_ldpc_rate_t rate,
                                                    poporon_ldpc_matrix_type_t matrix_type, uint32_t column_weight,
                                                    bool use_soft_decode, bool use_outer_interleave,
                                                    bool use_inner_interleave, uint32_t interleave_depth,
                                                    uint32_t lifting_factor, uint32_t max_iterations,
                                                    const int8_t *soft_llr, size_t soft_llr_size, uint64_t seed)
{
    poporon_config_t *c = (poporon_config_t *)calloc(1, sizeof(poporon_config_t));
    if (!c)
        return nullptr;
    c->fec_type = PPLN_FEC_LDPC;
    c->block_size = block_size;
    c->rate = (uint32_t)rate;
    c->matrix_type = (uint32_t)matrix_type;
    c->column_weight = column_weight;
    c->use_soft_decode = use_soft_decode;
    c->use_outer_interleave = use_outer_interleave;
    c->use_inner_interleave = use_inner_interleave;
    c->interleave_depth = interleave_depth;
    c->lifting_factor = lifting_factor;
    c->max_iterations = max_iterations;
    c->soft_llr = soft_llr;
    c->soft_llr_size = soft_llr_size;
    c->seed = seed;
    return c;
}
EXPORT poporon_config_t *poporon_bch_config_create(uint8_t symbol_size, uint16_t generator_polynomial,
                                                   uint8_t correction_capability)
{
    poporon_config_t *c = (poporon_config_t *)calloc(1, sizeof(poporon_config_t));
    if (!c)
        return nullptr;
    c->fec_type = PPLN_FEC_BCH;
    c->symbol_size = symbol_size;
    c->generator_polynomial = generator_polynomial;
    c->correction_capability = correction_capability;
    return c;
}
/* The two LDPC convenience constructors stay stubs (tests/test_library_cpu.py
 * pins their NULL): poporon_ldpc_config_create(block, rate, PPRN_LDPC_RANDOM,
 * 3 (default) or 7 (burst resistant), true, true, true, 0, 0, 0, NULL, 0, 0)
 * is what the reference's build (src/poporon.c:286-294). */
EXPORT poporon_config_t *poporon_config_ldpc_default(size_t, poporon_ldpc_rate_t)
{
    fail("poporon_config_ldpc_default is a stub: use poporon_ldpc_config_create (include/poporon.h)");
    return nullptr;
}
EXPORT poporon_config_t *poporon_config_ldpc_burst_resistant(size_t, poporon_ldpc_rate_t)
{
    fail("poporon_config_ldpc_burst_resistant is a stub: use poporon_ldpc_config_create (include/poporon.h)");
    return nullptr;
}
EXPORT poporon_config_t *poporon_config_bch_default(void) { return poporon_bch_config_create(4, 0x13, 3); }

EXPORT void poporon_config_destroy(poporon_config_t *config) { free(config); }

/* ------------------------------------------------------------------------ */
/* handle                                                                   */
/* ------------------------------------------------------------------------ */

static void build_decode_tables(poporon_t *h, uint32_t nr);

/* Kernel tables for the handle (see rs_device.h for their definitions). */
static void build_tables(poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    const poporon_gf_t *gf = rs->gf;
    const uint16_t *g = rs->generator_polynomial;
    RsDevTables &t = h->host_tab;
    memset(&t, 0, sizeof(t));
    uint8_t row[32];
    for (uint32_t fb = 0; fb < 256; fb++) {
        for (uint32_t m = 0; m < 32; m++)
            row[m] = fb == 0 ? 0
                             : (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[fb] + g[RS_NR - 1 - m]))];
        uint32_t il[8]; /* interleaved: dword k = row bytes k, k+8, k+16, k+24 */
        for (uint32_t k = 0; k < 8; k++)
            il[k] = (uint32_t)row[k] | ((uint32_t)row[k + 8] << 8) | ((uint32_t)row[k + 16] << 16) |
                    ((uint32_t)row[k + 24] << 24);
        memcpy(&t.lfsr[fb * 2], il, 16);
        memcpy(&t.lfsr[fb * 2 + 1], il + 4, 16);
    }
    /* encq: the LFSR above run on the message 1, 0, 0, ... (rs_enc1_k) */
    {
        uint8_t q[RS_NR];
        for (uint32_t m = 0; m < RS_NR; m++) /* one step with feedback 1 */
            q[m] = (uint8_t)gf->log2exp[gf_mod(gf, g[RS_NR - 1 - m])];
        for (uint32_t d = 0; d < 223; d++) {
            for (uint32_t m = 0; m < RS_NR; m++)
                t.encq[d * RS_NR + m] = (uint8_t)gf->exp2log[q[m]];
            const uint32_t fb = q[0]; /* next step, input byte 0 */
            for (uint32_t m = 0; m < RS_NR; m++) {
                const uint8_t sh = m + 1 < RS_NR ? q[m + 1] : 0;
                q[m] = sh ^ (fb == 0 ? 0
                                     : (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[fb] + g[RS_NR - 1 - m]))]);
            }
        }
    }
    build_decode_tables(h, RS_NR);
}

/* Everything but the LFSR rows and encq, for a code of nr <= 32 roots: GF
 * tables, decode parameters, E' -> syndrome nibble tables, Chien rows, the
 * split kernels' GF image.  For nr < 32, E' sits in the first nr register
 * bytes (byte m = coefficient of x^(nr-1-m), zeros behind) and the tables
 * give S_0..S_(nr-1), zeros behind them. */
static void build_decode_tables(poporon_t *h, uint32_t nr)
{
    const poporon_rs_t *rs = h->rs;
    const poporon_gf_t *gf = rs->gf;
    RsDevTables &t = h->host_tab;
    for (uint32_t x = 0; x < 512; x++)
        t.exp2[x] = (uint8_t)gf->log2exp[x % 255];
    t.exp2[511] = 0; /* ZLOG sentinel of the correction kernel (no sum of two logs reaches 511) */
    for (uint32_t v = 0; v < 256; v++)
        t.log[v] = (uint8_t)gf->exp2log[v];

    RsCorrParams &p = h->corr;
    memset(&p, 0, sizeof(p));
    p.fcr = rs->first_consecutive_root;
    p.prim = rs->primitive_element;
    p.iprim = h->primitive_inverse;
    p.vfast = ((uint64_t)(p.fcr + nr - 1) * p.prim * 254u) < 32768u;
    p.nr = nr;

    /* E' -> syndrome nibble tables (rs_device.h) */
    auto gmul = [&](uint32_t x, uint32_t logc) -> uint8_t {
        return x == 0 ? 0 : (uint8_t)gf->log2exp[(gf->exp2log[x] + logc) % 255];
    };
    for (uint32_t m = 0; m < RS_NR; m++) {
        for (uint32_t n = 0; n < 2; n++) {
            for (uint32_t v = 0; v < 16; v++) {
                uint8_t rowb[RS_NR];
                for (uint32_t i = 0; i < RS_NR; i++) {
                    if (m >= nr || i >= nr) {
                        rowb[i] = 0;
                        continue;
                    }
                    const uint64_t e = (uint64_t)(nr - 1 - m) * p.prim * (p.fcr + i);
                    rowb[i] = gmul(v << (4 * n), (uint32_t)(e % 255));
                }
                memcpy(&t.synt[((m * 2 + n) * 2 + 0) * 16 + v], rowb, 16);
                memcpy(&t.synt[((m * 2 + n) * 2 + 1) * 16 + v], rowb + 16, 16);
            }
        }
    }
    /* Chien chunk rows: term j at 16 consecutive points */
    for (uint32_t j = 1; j <= 32; j++) {
        for (uint32_t e = 0; e < 256; e++) {
            uint8_t rowb[16];
            for (uint32_t b = 0; b < 16; b++)
                rowb[b] = e == 255 ? 0 : (uint8_t)gf->log2exp[(e + j * b) % 255];
            memcpy(&t.chien[(j - 1) * 256 + e], rowb, 16);
        }
    }
    /* the split kernels' GF table image (rs_device.h) */
    uint32_t *gfa = reinterpret_cast<uint32_t *>(t.gfa);
    for (uint32_t x = 0; x < 512; x++)
        for (uint32_t r = 0; r < 32; r++) {
            const uint32_t la = x < 256u ? (x ? (uint32_t)t.log[x] * 128u + 4u * r + 1u : 128u * RS_Z0 + 4u * r) : 0u;
            gfa[x * 32 + r] = ((uint32_t)t.exp2[x] << 8) | (la << 16);
        }
    uint32_t *gfc = reinterpret_cast<uint32_t *>(t.gfc);
    for (uint32_t x = 0; x < 512; x++)
        for (uint32_t r = 0; r < 32; r++) {
            const uint32_t v = x & 255u;
            gfc[x * 32 + r] = ((uint32_t)t.exp2[x] << 8) | ((v ? (uint32_t)t.log[v] * 128u : 0xFFFFu) << 16);
        }
    const char *fv = getenv("POPORON_AMD_FORCE_VERIFY");
    p.force_verify = (fv && fv[0] == '1') ? 1u : 0u;
    const char *dp = getenv("POPORON_AMD_DECODE_PATH");
    h->decode_path = !dp ? 0 : !strcmp(dp, "split") ? 1 : !strcmp(dp, "single") ? 2 : !strcmp(dp, "wave") ? 3 : 0;
    const char *dt = getenv("POPORON_AMD_DECODE_TAIL");
    h->decode_tail = dt && !strcmp(dt, "split")    ? 1
                     : dt && !strcmp(dt, "fused")  ? 0
                     : dt && !strcmp(dt, "search") ? 2
                     : h->decode_path == 1         ? 1
                                                   : 3;
}

/* General-parameter kernels: byte symbols (2 <= m <= 8) and 1 <= num_roots
 * < 2^m - 1 (at least one message byte); every field polynomial, fcr and
 * prim that poporon_create accepts. */
static bool params_generic(const poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    const uint32_t m = rs->gf->symbol_size, nn = rs->gf->field_size;
    return m >= 2 && m <= 8 && rs->num_roots >= 1 && rs->num_roots < nn && rs->primitive_element != 0;
}

static void build_generic(poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    const poporon_gf_t *gf = rs->gf;
    RsGenTables &t = h->gen_tab;
    const uint32_t nn = gf->field_size;
    memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < 256; i++) {
        t.alog[i] = i <= nn ? (uint8_t)gf->log2exp[i] : 0;
        t.log[i] = i <= nn ? (uint8_t)gf->exp2log[i] : (uint8_t)nn;
    }
    for (uint32_t i = 0; i <= rs->num_roots; i++)
        t.gen[i] = (uint8_t)rs->generator_polynomial[i];
    /* lrow: the rows of rsg_lfsr_k (rs_generic.h) */
    for (uint32_t fb = 0; fb < 256; fb++) {
        const uint32_t v = fb & nn;
        for (uint32_t i = 0; i < rs->num_roots && v != 0; i++)
            t.lrow[fb * 256 + i] = (uint8_t)gf->log2exp[gf_mod(
                gf, (uint16_t)(gf->exp2log[v] + rs->generator_polynomial[rs->num_roots - 1 - i]))];
    }
    /* encq: the register after each byte of the message 1, 0, 0, ... -- the
     * steps of src/encode.c:120-143 as rsg_encode_k takes them (the
     * generator's logs used as they are) */
    {
        const uint32_t nr = rs->num_roots;
        const uint16_t *g = rs->generator_polynomial;
        memset(t.encq, 0xff, sizeof(t.encq));
        std::vector<uint8_t> reg(nr, 0);
        for (uint32_t d = 0; d < nn - nr; d++) {
            const uint32_t fb = gf->exp2log[(d == 0 ? 1u : 0u) ^ reg[0]];
            if (fb != nn)
                for (uint32_t j = 1; j < nr; j++)
                    reg[j] ^= (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(fb + g[nr - j]))];
            for (uint32_t j = 0; j + 1 < nr; j++)
                reg[j] = reg[j + 1];
            reg[nr - 1] = fb != nn ? (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(fb + g[0]))] : 0;
            for (uint32_t j = 0; j < nr; j++)
                t.encq[d * 256 + j] = reg[j] ? (uint8_t)gf->exp2log[reg[j]] : (uint8_t)0xff;
        }
    }
    RsGenParams &p = h->gen;
    memset(&p, 0, sizeof(p));
    p.m = gf->symbol_size;
    p.nn = nn;
    p.magic = (uint32_t)((1ull << 32) / nn) + 1u;
    p.fcr = rs->first_consecutive_root;
    p.prim = rs->primitive_element;
    p.iprim = h->primitive_inverse;
    p.nroots = rs->num_roots;
}

static bool params_supported(const poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    if (rs->gf->symbol_size != 8 || rs->num_roots != RS_NR || rs->primitive_element == 0)
        return false;
    if (((uint32_t)rs->first_consecutive_root + RS_NR - 1) * rs->primitive_element + 254u >= 65536u)
        return false;
    /* distinct roots: then "remainder == 0" <=> "all syndromes are zero" */
    const uint32_t p = rs->primitive_element;
    if (p % 3 == 0 || p % 5 == 0 || p % 17 == 0)
        return false;
    for (uint32_t i = 0; i < RS_NR; i++) /* the LFSR remainder needs a generator without zero coefficients */
        if (rs->generator_polynomial[i] == rs->gf->field_size)
            return false;
    return true;
}

/* Codes with at most 32 roots encode on the RS(255,223) LFSR kernel with
 * g'(x) = g(x) x^(32 - nr) (rsk_encode_nr, rs_kernels.hip; 32 roots: the
 * codes the fast path leaves to the general kernels): the same steps as
 * src/encode.c:120-143 on the first nr register bytes, zeros behind them.
 * Symbols of m < 8 bits too: the register bytes stay below 2^m, so the
 * reference's feedback log[(d & nn) ^ p_0] is row (d ^ p_0) & nn, and the
 * rows of feedback bytes >= 2^m repeat those of their low m bits
 * (build_lfsr_rows).  Like the fast path it needs a generator without zero
 * coefficients (the reference's log-form LFSR reads a zero coefficient's log
 * literally). */
static bool params_lfsr_nr(const poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    if (rs->gf->symbol_size > 8 || rs->num_roots == 0 || rs->num_roots > RS_NR || rs->primitive_element == 0)
        return false;
    for (uint32_t i = 0; i < rs->num_roots; i++)
        if (rs->generator_polynomial[i] == rs->gf->field_size)
            return false;
    return true;
}

/* Byte-symbol codes with 2 <= nr < 32 roots decode large error-mode batches
 * on the split kernels (rsk_syndrome_reset_nr .. rsk_apply_nr, the list on
 * the general kernel): the LFSR conditions above, distinct roots (prim
 * coprime to 255: "remainder zero" <=> "all syndromes zero") and the fast
 * path's exponent bound, as params_supported. */
static bool params_nrsplit(const poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    if (!params_lfsr_nr(h) || rs->gf->symbol_size != 8 || rs->num_roots < 2 || rs->num_roots >= RS_NR)
        return false; /* GF(2^8) split kernels with npar < 32 (32 roots: the fast path's own codes) */
    const uint32_t p = rs->primitive_element;
    if (p % 3 == 0 || p % 5 == 0 || p % 17 == 0)
        return false;
    return ((uint32_t)rs->first_consecutive_root + rs->num_roots - 1) * p + 254u < 65536u;
}

/* rows of g'(x) = g(x) x^(32 - nr) in the LFSR kernel's interleaved layout:
 * row byte m = fb * g_(nr-1-m) for m < nr (src/encode.c:126-140), 0 past it;
 * feedback byte fb selects the row of fb & nn (m < 8: params_lfsr_nr) */
static void build_lfsr_rows(poporon_t *h)
{
    const poporon_rs_t *rs = h->rs;
    const poporon_gf_t *gf = rs->gf;
    const uint16_t *g = rs->generator_polynomial;
    const uint32_t nr = rs->num_roots;
    RsDevTables &t = h->host_tab;
    memset(&t, 0, sizeof(t));
    uint8_t row[32];
    for (uint32_t fb = 0; fb < 256; fb++) {
        const uint32_t v = fb & gf->field_size;
        for (uint32_t m = 0; m < 32; m++)
            row[m] = (v == 0 || m >= nr)
                         ? 0
                         : (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[v] + g[nr - 1 - m]))];
        uint32_t il[8];
        for (uint32_t k = 0; k < 8; k++)
            il[k] = (uint32_t)row[k] | ((uint32_t)row[k + 8] << 8) | ((uint32_t)row[k + 16] << 16) |
                    ((uint32_t)row[k + 24] << 24);
        memcpy(&t.lfsr[fb * 2], il, 16);
        memcpy(&t.lfsr[fb * 2 + 1], il + 4, 16);
    }
    /* encq: parity (log form, 255 = zero, stride 32) of the message 1 followed
     * by d zeros, d < 255 - nr: the same LFSR steps (rs_enc1_k) */
    memset(t.encq, 255, sizeof(t.encq));
    uint8_t q[RS_NR];
    for (uint32_t m = 0; m < nr; m++) /* one step with feedback 1 */
        q[m] = (uint8_t)gf->log2exp[gf_mod(gf, g[nr - 1 - m])];
    for (uint32_t d = 0; d < 255u - nr; d++) {
        for (uint32_t m = 0; m < nr; m++)
            t.encq[d * RS_NR + m] = (uint8_t)gf->exp2log[q[m]];
        const uint32_t fb = q[0]; /* next step, input byte 0 */
        for (uint32_t m = 0; m < nr; m++) {
            const uint8_t sh = m + 1 < nr ? q[m + 1] : 0;
            q[m] = sh ^ (fb == 0 ? 0 : (uint8_t)gf->log2exp[gf_mod(gf, (uint16_t)(gf->exp2log[fb] + g[nr - 1 - m]))]);
        }
    }
}

/* ---- BCH handle: generator from minimal polynomials (src/bch.c:184-285) ---- */
static uint32_t bch_min_poly(const poporon_gf_t *gf, uint32_t e)
{
    uint16_t p[64];
    uint32_t deg = 0, c = e, out = 0;
    memset(p, 0, sizeof(p));
    p[0] = 1;
    do {
        const uint16_t root = gf->log2exp[c];
        for (int j = (int)deg; j >= 0; j--) {
            if (j + 1 < 64)
                p[j + 1] ^= p[j];
            p[j] = (p[j] && root) ? gf->log2exp[(gf->exp2log[p[j]] + gf->exp2log[root]) % gf->field_size] : 0;
        }
        deg++;
        c = (c * 2) % gf->field_size;
    } while (c != e);
    for (uint32_t i = 0; i <= deg && i < 32; i++)
        if (p[i] == 1)
            out |= 1u << i;
    return out;
}

static poporon_t *create_bch(const poporon_config_t *config)
{
    const uint32_t m = config->symbol_size, t = config->correction_capability;
    if (m < 3 || m > 16 || t < 1 || t > 16) /* src/bch.c:290-296 */
        return nullptr;
    poporon_gf_t *gf = poporon_gf_create(config->symbol_size, config->generator_polynomial);
    if (!gf)
        return nullptr;
    poporon_t *h = new (std::nothrow) _poporon_t();
    if (!h) {
        poporon_gf_destroy(gf);
        return nullptr;
    }
    h->fec_type = PPLN_FEC_BCH;
    h->rs = nullptr;
    h->bgf = gf;
    BchParams &b = h->bch;
    memset(&b, 0, sizeof(b));
    b.m = m;
    b.nn = gf->field_size;
    b.t = t;
    /* codewords of more than 31 bits overflow the reference's uint32 shifts
     * (undefined behaviour): the handle exists, its codec calls fail */
    h->bch_ok = m <= 5;
    if (h->bch_ok) {
        std::vector<uint8_t> used(b.nn + 1, 0);
        uint32_t gen = 1, gdeg = 0;
        for (uint32_t i = 1; i <= 2 * t; i++) {
            const uint32_t e = i % b.nn;
            if (used[e])
                continue;
            uint32_t c = e;
            do {
                used[c] = 1;
                c = (c * 2) % b.nn;
            } while (c != e);
            const uint32_t mp = bch_min_poly(gf, e);
            uint32_t prod = 0;
            for (uint32_t j = 0; j <= gdeg; j++)
                if (gen & (1u << j))
                    prod ^= mp << j;
            gen = prod;
            gdeg = 31u - (uint32_t)__builtin_clz(gen);
        }
        b.gen = gen;
        b.gdeg = gdeg;
        b.pbits = gdeg;
        b.k = b.nn - gdeg;
        b.dbytes = (b.k + 7) / 8;
        b.pbytes = (b.pbits + 7) / 8;
        for (uint32_t i = 0; i < 32; i++) {
            b.alog[i] = i <= b.nn ? (uint8_t)gf->log2exp[i] : 0;
            b.log[i] = i <= b.nn ? (uint8_t)gf->exp2log[i] : 0;
        }
    }
    return h;
}

/* src/poporon.c:112-146 over poporon_ldpc_create (src/ldpc.c:814-872): the
 * graph is built on the host (ldpc_graph.cpp), no GPU needed.  A code whose
 * inner interleaver is no permutation exists, answers the getters and fails
 * every codec call (the reference decodes it through uninitialised memory). */
static poporon_t *create_ldpc(const poporon_config_t *config)
{
    LdpcGraph *lg = new (std::nothrow) LdpcGraph();
    if (!lg)
        return nullptr;
    if (!ldpc_graph_build(*lg, config->block_size, config->rate, config->matrix_type, config->column_weight,
                          config->use_outer_interleave, config->use_inner_interleave, config->interleave_depth,
                          config->lifting_factor, config->seed)) {
        delete lg;
        return nullptr;
    }
    poporon_t *h = new (std::nothrow) _poporon_t();
    if (!h) {
        delete lg;
        return nullptr;
    }
    h->fec_type = PPLN_FEC_LDPC;
    h->rs = nullptr;
    h->ldpc = lg;
    h->ldpc_max_iterations = config->max_iterations;
    h->ldpc_soft = config->use_soft_decode;
    h->ldpc_llr = config->soft_llr;
    h->ldpc_last_iterations = 0;
    h->supported = !lg->inner || lg->inner_bijective;
    const char *lp = getenv("POPORON_AMD_LDPC_PATH");
    h->ldpc_path = !lp ? 0 : !strcmp(lp, "lds") ? 1 : !strcmp(lp, "global") ? 2 : 0;
    LdpcDev &v = h->ldev;
    memset(&v, 0, sizeof(v));
    v.info_bits = lg->info_bits;
    v.parity_bits = lg->parity_bits;
    v.codeword_bits = lg->codeword_bits;
    v.info_bytes = lg->info_bytes;
    v.parity_bytes = lg->parity_bytes;
    v.codeword_bytes = lg->codeword_bytes;
    v.num_checks = lg->num_checks;
    v.num_bits = lg->num_bits;
    v.num_edges = lg->num_edges;
    return h;
}

EXPORT poporon_t *poporon_create(const poporon_config_t *config)
{
    if (!config)
        return nullptr;
    if (config->fec_type == PPLN_FEC_BCH)
        return create_bch(config);
    if (config->fec_type == PPLN_FEC_LDPC)
        return create_ldpc(config);
    if (config->fec_type != PPLN_FEC_RS)
        return nullptr;
    poporon_rs_t *rs = poporon_rs_create(config->symbol_size, config->generator_polynomial,
                                         config->first_consecutive_root, config->primitive_element, config->num_roots);
    if (!rs)
        return nullptr;
    if (config->primitive_element == 0) {
        poporon_rs_destroy(rs);
        return nullptr;
    }
    /* smallest 1 + j*field_size (uint16 arithmetic) divisible by prim, over prim */
    uint32_t tries = 0;
    uint16_t pi;
    for (pi = 1; (pi % config->primitive_element) != 0; pi = (uint16_t)(pi + rs->gf->field_size)) {
        if (++tries > (uint32_t)rs->gf->field_size * 2) {
            poporon_rs_destroy(rs);
            return nullptr;
        }
    }
    poporon_t *h = new (std::nothrow) _poporon_t();
    if (!h) {
        poporon_rs_destroy(rs);
        return nullptr;
    }
    h->fec_type = PPLN_FEC_RS;
    h->rs = rs;
    h->primitive_inverse = (uint16_t)(pi / config->primitive_element);
    h->erasure = config->erasure;
    h->ext_syndrome = config->syndrome;
    h->last_corrected = 0;
    h->fast = params_supported(h);
    h->generic = !h->fast && params_generic(h);
    h->lfsr_nr = h->generic && params_lfsr_nr(h);
    h->nrsplit = h->lfsr_nr && params_nrsplit(h);
    h->supported = h->fast || h->generic;
    {
        const char *gp = getenv("POPORON_AMD_GENERIC");
        h->gen_path = !gp ? 0 : !strcmp(gp, "lane") ? 1 : !strcmp(gp, "wave") ? 2 : 0;
    }
    {
        const char *ic = getenv("POPORON_AMD_ILV_CHUNK");
        const unsigned long long v = ic ? strtoull(ic, nullptr, 10) : 0ull;
        h->ilv_chunk = v ? (size_t)std::min<unsigned long long>(v, ILV_CHUNK_MAX) : ILV_CHUNK_DEFAULT;
    }
    {
        const char *rc = getenv("POPORON_AMD_REPORT_CHUNK");
        const unsigned long long v = rc ? strtoull(rc, nullptr, 10) : 0ull;
        h->rep_chunk = v ? (size_t)std::min<unsigned long long>(v, REP_CHUNK_MAX) : REP_CHUNK_DEFAULT;
    }
    {
        const char *cp = getenv("POPORON_AMD_CONV_PATH");
        h->conv_path = !cp                    ? RS_CONV_PATH_AUTO
                       : !strcmp(cp, "tile")   ? RS_CONV_PATH_TILE
                       : !strcmp(cp, "direct") ? RS_CONV_PATH_DIRECT
                                               : RS_CONV_PATH_AUTO;
    }
    if (h->fast)
        build_tables(h);
    if (h->generic)
        build_generic(h);
    if (h->lfsr_nr)
        build_lfsr_rows(h);
    if (h->nrsplit)
        build_decode_tables(h, rs->num_roots);
    return h;
}

/* The next request word of the single-call server (rs_serve_k): a new
 * sequence number, and never the word the server saw last -- it acts on a
 * change of the word only (14 bits of sequence wrap). */
static uint32_t srv_word(GpuCtx &g, uint32_t prev, uint32_t op, uint32_t size, uint32_t mode)
{
    uint32_t w;
    do
        w = ZC_REQ_WORD(++g.srv_seq, op, size, mode);
    while (w == prev);
    return w;
}

/* Scoped switch to the handle's device; restores the caller's device. */
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

/* ------------------------------------------------------------------------ */
/* Handles per device: a batch call and other handles' single-call servers   */
/* ------------------------------------------------------------------------ */

/* A resident single-call server (rs_serve_k / rsgw_serve_k) holds one CU's
 * LDS; a persistent batch grid (rs_lfsr_k: one 128-160 KB workgroup per CU)
 * launched beside it waits for that CU until the server leaves (its idle
 * limit, 1 ms, or 0.5 s while its handle keeps calling).  A batch call stops
 * its own handle's server (srv_stop); the registry below makes the servers of
 * the other handles on the device leave too (yield_servers bumps their
 * ZC_YIELD word, which every server polls with its request word), and keeps
 * them from relaunching while the batch has not run (srv_may_launch): such a
 * single call is served by one launch instead (rs_dec1_k / rs_enc1_k /
 * rsgw_*_k), a kernel that ends on its own.  The reference's handles share
 * nothing (src/poporon.c, no globals); this keeps a handle's batch
 * throughput independent of another thread's single calls. */
#define MAX_DEVS 64
struct DevRegistry {
    std::mutex mu;
    std::vector<GpuCtx *> ctx;
};
static DevRegistry g_devs[MAX_DEVS];

static void dev_register(GpuCtx &g)
{
    if (g.registered || g.device < 0 || g.device >= MAX_DEVS)
        return;
    std::lock_guard<std::mutex> lk(g_devs[g.device].mu);
    g_devs[g.device].ctx.push_back(&g);
    g.registered = true;
}

static void dev_unregister(GpuCtx &g)
{
    if (!g.registered)
        return;
    DevRegistry &r = g_devs[g.device];
    std::lock_guard<std::mutex> lk(r.mu);
    r.ctx.erase(std::remove(r.ctx.begin(), r.ctx.end(), &g), r.ctx.end());
    g.registered = false;
}

/* batch_enter: with other handles on the device, mark this batch open and
 * ask their servers to leave */
static void yield_servers(GpuCtx &g)
{
    if (!g.registered)
        return;
    DevRegistry &r = g_devs[g.device];
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.ctx.size() < 2)
        return;
    g.batch_open = true;
    for (GpuCtx *x : r.ctx)
        if (x != &g && x->zc) {
            volatile uint32_t *y = reinterpret_cast<volatile uint32_t *>(x->zc + ZC_YIELD);
            *y = *y + 1u;
        }
}

/* the end of a batch call: its completion event behind its launches on
 * `stream` (synchronous calls: none) */
static void batch_exit(GpuCtx &g, hipStream_t stream, bool sync)
{
    if (!g.batch_open)
        return;
    DeviceGuard dg(g.device);
    std::lock_guard<std::mutex> lk(g_devs[g.device].mu);
    g.batch_open = false;
    if (sync)
        return;
    if (!g.batch_ev && hipEventCreateWithFlags(&g.batch_ev, hipEventDisableTiming) != hipSuccess) {
        g.batch_ev = nullptr;
        return;
    }
    g.batch_ev_live = hipEventRecord(g.batch_ev, stream) == hipSuccess;
}

struct BatchScope {
    GpuCtx &g;
    hipStream_t stream;
    bool sync;
    ~BatchScope() { batch_exit(g, stream, sync); }
};

/* Frees whatever the context holds, ready or not: a gpu_init that failed
 * half-way leaves a stream or tables behind, and they go here so that the
 * next call retries from scratch. */
static void gpu_release(GpuCtx &g)
{
    const int dev = g.device;
    const bool any = g.ready || g.stream || g.sstream || g.tab || g.gtab || g.rem || g.ltab || g.lws || g.stage ||
                     g.hstage || g.zc || g.ilv.p || g.rep.p || g.plist.p || g.soft.p || g.wire || g.rslot.stream ||
                     g.rem_done || g.registered || g.batch_ev ||
                     g.pipe[0].stream || g.pipe[1].stream || g.pipe[2].stream;
    if (!any || dev < 0) {
        g = GpuCtx();
        g.device = dev;
        return;
    }
    dev_unregister(g); /* no other handle touches g.zc or the batch state from here on */
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
    if (g.stream)
        (void)hipStreamSynchronize(g.stream);
    if (g.batch_ev)
        (void)hipEventDestroy(g.batch_ev);
    if (g.rem_done) {
        (void)hipEventSynchronize(g.rem_done);
        (void)hipEventDestroy(g.rem_done);
    }
    for (auto &t : g.pending) {
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    for (auto e : g.event_pool)
        (void)hipEventDestroy(e);
    (void)hipFree(g.tab);
    (void)hipFree(g.gtab);
    (void)hipFree(g.rem);
    for (DevBuf *b : {&g.ilv, &g.rep, &g.plist, &g.soft})
        (void)hipFree(b->p);
    (void)hipFree(g.wire);
    (void)hipFree(g.ltab);
    (void)hipFree(g.lws);
    (void)hipFree(g.stage);
    if (g.hstage)
        (void)hipHostFree(g.hstage);
    if (g.sstream) {
        if (g.zc && g.srv_on) { /* ask a live server to leave now rather than at its idle limit */
            volatile uint32_t *req = reinterpret_cast<volatile uint32_t *>(g.zc + ZC_REQ);
            *req = srv_word(g, *req, RS_SRV_STOP, 0u, 0u);
        }
        (void)hipStreamSynchronize(g.sstream);
        (void)hipStreamDestroy(g.sstream);
    }
    if (g.zc)
        (void)hipHostFree(g.zc);
    for (GpuCtx::PipeSlot *slot : {&g.pipe[0], &g.pipe[1], &g.pipe[2], &g.rslot}) {
        GpuCtx::PipeSlot &ps = *slot;
        if (ps.stream)
            (void)hipStreamSynchronize(ps.stream);
        (void)hipHostFree(ps.host);
        (void)hipFree(ps.dev);
        if (ps.done)
            (void)hipEventDestroy(ps.done);
        if (ps.stream)
            (void)hipStreamDestroy(ps.stream);
    }
    if (g.stream)
        (void)hipStreamDestroy(g.stream);
    if (prev >= 0)
        (void)hipSetDevice(prev);
    g = GpuCtx();
    g.device = dev; /* a handle stays bound to the device it was given */
}

EXPORT void poporon_destroy(poporon_t *h)
{
    if (!h)
        return;
    gpu_release(h->gpu);
    poporon_rs_destroy(h->rs);
    poporon_gf_destroy(h->bgf);
    delete h->ldpc;
    delete h;
}

EXPORT poporon_fec_type_t poporon_get_fec_type(const poporon_t *h) { return h ? h->fec_type : PPLN_FEC_UNKNOWN; }
EXPORT uint32_t poporon_get_iterations_used(const poporon_t *h)
{
    return h && h->fec_type == PPLN_FEC_LDPC ? h->ldpc_last_iterations : 0;
}
/* src/poporon.c:322-362: BCH sizes are the byte images of the parity / data bits */
EXPORT size_t poporon_get_parity_size(const poporon_t *h)
{
    if (!h)
        return 0;
    if (h->fec_type == PPLN_FEC_BCH)
        return h->bch_ok ? h->bch.pbytes : 0;
    if (h->fec_type == PPLN_FEC_LDPC)
        return h->ldpc->parity_bytes;
    return h->rs->num_roots;
}
EXPORT size_t poporon_get_info_size(const poporon_t *h)
{
    if (!h)
        return 0;
    if (h->fec_type == PPLN_FEC_BCH)
        return h->bch_ok ? h->bch.dbytes : 0;
    if (h->fec_type == PPLN_FEC_LDPC)
        return h->ldpc->info_bytes;
    return (size_t)(h->rs->gf->field_size - h->rs->num_roots);
}
EXPORT uint32_t poporon_version_id(void) { return (uint32_t)POPORON_VERSION_ID; }
EXPORT poporon_buildtime_t poporon_buildtime(void) { return (poporon_buildtime_t)POPORON_BUILDTIME; }

/* ------------------------------------------------------------------------ */
/* GPU context                                                              */
/* ------------------------------------------------------------------------ */

EXPORT int poporon_amd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

EXPORT bool poporon_amd_supported(const poporon_t *h) { return h && h->supported; }


EXPORT bool poporon_amd_set_device(poporon_t *h, int device)
{
    if (!h)
        return fail("NULL handle");
    if (h->gpu.ready && h->gpu.device != device)
        return fail("handle already bound to device %d", h->gpu.device);
    int n = poporon_amd_device_count();
    if (device < 0 || device >= n)
        return fail("device %d out of range (%d HIP devices)", device, n);
    h->gpu.device = device;
    return true;
}

static bool gpu_init_steps(poporon_t *h);

/* Lazily binds the handle to its device and uploads its tables.  A failure
 * part-way releases what was created, so a later call can retry. */
static bool gpu_init(poporon_t *h)
{
    if (h->gpu.ready)
        return true;
    if (gpu_init_steps(h))
        return true;
    const std::string msg = g_last_error;
    gpu_release(h->gpu);
    g_last_error = msg;
    return false;
}

/* the single-call server (below) leaves before a batch call on its handle:
 * while resident it holds a CU (and, with few hardware queues, may sit ahead of
 * the batch's dispatches) */
static bool srv_stop(poporon_t *h);

/* every batch entry point: the device context, and no live server of this
 * handle beside the batch's kernels */
static bool batch_enter(poporon_t *h)
{
    if (!gpu_init(h) || !srv_stop(h))
        return false;
    yield_servers(h->gpu);
    return true;
}

/* the graph's tables in one device allocation; the launch parameters point into it */
static bool ldpc_upload(poporon_t *h)
{
    GpuCtx &g = h->gpu;
    const LdpcGraph &lg = *h->ldpc;
    const std::vector<uint32_t> *src[8] = {&lg.row_ptr,       &lg.col_idx,       &lg.col_ptr,       &lg.edge_idx,
                                           &lg.inner_forward, &lg.inner_inverse, &lg.outer_forward, &lg.outer_inverse};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; i++) {
        off[i] = total;
        total += (src[i]->size() + 3) & ~(size_t)3;
    }
    HIP_OK(hipMalloc((void **)&g.ltab, total * sizeof(uint32_t)));
    const uint32_t *dev[8];
    for (int i = 0; i < 8; i++) {
        dev[i] = src[i]->empty() ? nullptr : g.ltab + off[i];
        if (!src[i]->empty())
            HIP_OK(hipMemcpy(g.ltab + off[i], src[i]->data(), src[i]->size() * sizeof(uint32_t),
                             hipMemcpyHostToDevice));
    }
    LdpcDev &v = h->ldev;
    v.row_ptr = dev[0];
    v.col_idx = dev[1];
    v.col_ptr = dev[2];
    v.edge_idx = dev[3];
    v.inner_forward = dev[4];
    v.inner_inverse = dev[5];
    v.outer_forward = dev[6];
    v.outer_inverse = dev[7];
    return true;
}

static bool gpu_init_steps(poporon_t *h)
{
    GpuCtx &g = h->gpu;
    if (h->fec_type == PPLN_FEC_BCH && !h->bch_ok)
        return fail("BCH codewords longer than 31 bits (symbol_size > 5) are not served");
    if (h->fec_type == PPLN_FEC_LDPC && !h->supported)
        return fail("LDPC inner interleaver is not a permutation (depth * width != codeword_bits): the reference "
                    "decodes such a code through uninitialised memory; not served");
    if (h->fec_type == PPLN_FEC_RS && !h->supported)
        return fail("RS parameters not served by the GPU kernels (need 2 <= symbol_size <= 8 and "
                    "1 <= num_roots < 2^symbol_size - 1)");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail("no HIP device available (%s); libpoporon_amd has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "0 devices");
    if (g.device < 0) {
        int cur = 0;
        HIP_OK(hipGetDevice(&cur));
        g.device = cur;
    }
    DeviceGuard dg(g.device);
    if (!dg.ok)
        return fail("hipSetDevice(%d) failed", g.device);
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, g.device));
    g.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_OK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&g.rem_done, hipEventDisableTiming));
    if (h->fec_type == PPLN_FEC_BCH) {
        /* parameters and tables go by value with every launch */
    } else if (h->fec_type == PPLN_FEC_LDPC) {
        if (!ldpc_upload(h))
            return false;
    } else if (h->fast) {
        HIP_OK(hipMalloc((void **)&g.tab, sizeof(RsDevTables)));
        HIP_OK(hipMemcpy(g.tab, &h->host_tab, sizeof(RsDevTables), hipMemcpyHostToDevice));
    } else {
        HIP_OK(hipMalloc((void **)&g.gtab, sizeof(RsGenTables)));
        HIP_OK(hipMemcpy(g.gtab, &h->gen_tab, sizeof(RsGenTables), hipMemcpyHostToDevice));
        if (h->lfsr_nr) { /* the LFSR rows of g(x) x^(32 - nr) (+ the split decode's tables: nrsplit) */
            HIP_OK(hipMalloc((void **)&g.tab, sizeof(RsDevTables)));
            HIP_OK(hipMemcpy(g.tab, &h->host_tab, sizeof(RsDevTables), hipMemcpyHostToDevice));
        }
    }
    g.ready = true;
    dev_register(g);
    return true;
}

static bool ensure_rem(poporon_t *h, size_t count)
{
    GpuCtx &g = h->gpu;
    if (g.rem_cap >= count)
        return true;
    size_t cap = std::max(count, (size_t)1024);
    if (g.rem) {
        /* the last reader of rem may run on any stream the caller chose */
        if (g.rem_pending)
            HIP_OK(hipEventSynchronize(g.rem_done));
        g.rem_pending = false;
        HIP_OK(hipStreamSynchronize(g.stream));
        HIP_OK(hipFree(g.rem));
        g.rem = nullptr;
        g.rem_cap = 0;
    }
    HIP_OK(hipMalloc((void **)&g.rem, rs_ws_bytes(cap)));
    g.rem_cap = cap;
    return true;
}

/* b anew with cap units of unit_bytes; the caller has waited for its readers */
static bool buf_renew(DevBuf &b, size_t cap, size_t unit_bytes)
{
    HIP_OK(hipFree(b.p));
    b = DevBuf();
    HIP_OK(hipMalloc((void **)&b.p, cap * unit_bytes));
    b.cap = cap;
    return true;
}

/* The handle's buffers that the layout forms share across streams under rem's
 * ordering (ilv, rep, plist, soft): at least `units` units of unit_bytes, min_units
 * when it is allocated at all.  The last reader of the old buffer may run on
 * any stream the caller chose: wait for it before the free. */
static bool ensure_buf(GpuCtx &g, DevBuf &b, size_t units, size_t unit_bytes, size_t min_units)
{
    if (b.cap >= units)
        return true;
    if (b.p) {
        if (g.rem_pending)
            HIP_OK(hipEventSynchronize(g.rem_done));
        g.rem_pending = false;
    }
    return buf_renew(b, std::max(units, min_units), unit_bytes);
}

static bool ensure_stage(poporon_t *h, size_t bytes)
{
    GpuCtx &g = h->gpu;
    if (g.stage_cap >= bytes)
        return true;
    size_t cap = std::max(bytes, (size_t)4096);
    if (g.stage || g.hstage) {
        HIP_OK(hipStreamSynchronize(g.stream));
        HIP_OK(hipFree(g.stage));
        if (g.hstage)
            HIP_OK(hipHostFree(g.hstage));
        g.stage = nullptr;
        g.hstage = nullptr;
        g.stage_cap = 0;
    }
    HIP_OK(hipMalloc((void **)&g.stage, cap));
    HIP_OK(hipHostMalloc((void **)&g.hstage, cap, hipHostMallocDefault));
    g.stage_cap = cap;
    return true;
}

/* LDPC decode: messages in LDS (the forced or automatic choice), else in the workspace */
static bool ldpc_use_lds(const poporon_t *h)
{
    return h->ldpc_path == 1 || (h->ldpc_path == 0 && ldpck_decode_lds_bytes(&h->ldev) <= ldpck_decode_lds_room());
}

/* the workspace of a decode of `count` rows: one slice per workgroup of its launch */
static bool ldpc_reserve(poporon_t *h, size_t count)
{
    GpuCtx &g = h->gpu;
    if (ldpc_use_lds(h) || count == 0)
        return true;
    const size_t need = (size_t)ldpck_decode_grid(&h->ldev, count, g.num_cu, false) * ldpck_slice_bytes(&h->ldev);
    if (g.lws_bytes >= need)
        return true;
    if (g.lws) {
        if (g.rem_pending)
            HIP_OK(hipEventSynchronize(g.rem_done));
        g.rem_pending = false;
        HIP_OK(hipFree(g.lws));
        g.lws = nullptr;
        g.lws_bytes = 0;
    }
    HIP_OK(hipMalloc((void **)&g.lws, need));
    g.lws_bytes = need;
    return true;
}

EXPORT bool poporon_amd_reserve(poporon_t *h, size_t max_count)
{
    if (!h)
        return fail("NULL handle");
    if (!gpu_init(h))
        return false;
    DeviceGuard dg(h->gpu.device);
    if (h->fec_type == PPLN_FEC_LDPC)
        return ldpc_reserve(h, max_count);
    return ensure_rem(h, max_count);
}

/* the RS / BCH batch calls do not serve LDPC handles: those have entry points of their own */
static bool is_ldpc(const poporon_t *h, const char *what)
{
    if (h->fec_type != PPLN_FEC_LDPC)
        return false;
    fail("%s does not serve LDPC handles: use the poporon_ldpc_*_batch calls", what);
    return true;
}

/* parity bytes per codeword: num_roots (RS) or the BCH parity byte image */
static size_t par_bytes(const poporon_t *h)
{
    return h->fec_type == PPLN_FEC_BCH ? h->bch.pbytes : h->rs->num_roots;
}

/* largest decodable message size (RS: src/decode.c:418-429); BCH: no upper bound */
static size_t kmax(const poporon_t *h)
{
    return h->fec_type == PPLN_FEC_BCH ? (size_t)-1 : (size_t)h->rs->gf->field_size - h->rs->num_roots;
}

/* Encode sizes: the reference's uint16 byte counter never terminates past
 * 65535 (src/encode.c:121,125, quirk Q7: refused here); a BCH message must
 * hold the info byte image (src/encode.c:210-212). */
static bool check_encode_size(const poporon_t *h, size_t size)
{
    if (h->fec_type == PPLN_FEC_BCH && size < h->bch.dbytes)
        return fail("BCH encode size %zu < info byte image %u", size, (unsigned)h->bch.dbytes);
    if (size > 65535)
        return fail("size %zu > 65535 (the reference's uint16 byte counter never terminates)", size);
    return true;
}

static bool check_decode_size(const poporon_t *h, size_t size)
{
    if (h->fec_type == PPLN_FEC_BCH) /* src/decode.c:553-555, :598 */
        return size >= 1 && size >= h->bch.dbytes;
    /* src/decode.c:418-429: pad = nn - nroots - size must lie in [0, nn - nroots) */
    return size >= 1 && size <= kmax(h);
}

/* what every row decode entry point (host or device pointers) checks before
 * it touches the GPU; rs_only: the report calls, which serve RS handles alone */
static bool decode_row_args(const poporon_t *h, const char *what, bool rs_only, const uint8_t *data,
                            const uint8_t *parity, size_t size, size_t count, const uint8_t *positions,
                            size_t positions_stride, const uint8_t *counts, const uint8_t *ok)
{
    if (!h)
        return fail("%s: NULL handle", what);
    if (rs_only && h->fec_type != PPLN_FEC_RS)
        return fail("%s serves RS handles", what);
    if (is_ldpc(h, what))
        return false;
    if (count && (!data || !parity || !ok))
        return fail("%s: NULL argument", what);
    if (positions && (h->fec_type != PPLN_FEC_RS || !counts || positions_stride < h->rs->num_roots))
        return fail("%s: erasure batch needs an RS handle, counts and positions_stride >= num_roots", what);
    if (!check_decode_size(h, size))
        return fail("%s: decode size %zu outside [1, %u]", what, size, (unsigned)kmax(h));
    return true;
}

/* ------------------------------------------------------------------------ */
/* in-library kernel timing (HIP events on the launch stream)               */
/* ------------------------------------------------------------------------ */

static hipEvent_t take_event(GpuCtx &g)
{
    hipEvent_t e = nullptr;
    if (!g.event_pool.empty()) {
        e = g.event_pool.back();
        g.event_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}

/* Time the launches of one stage when timing is on: the events ride on the
 * kernels' own dispatches (RS_LAUNCH, rs_device.h) */
thread_local RsLaunchTimer rs_launch_timer = {nullptr, nullptr, 0};

struct KernelTimer {
    GpuCtx &g;
    int kernel;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(GpuCtx &g_, int k, hipStream_t) : g(g_), kernel(k)
    {
        if (!g.timing || (a = take_event(g)) == nullptr)
            return;
        if ((b = take_event(g)) == nullptr) {
            g.event_pool.push_back(a);
            a = nullptr;
            return;
        }
        rs_launch_timer = {a, b, 0};
    }
    /* every call site ends a successful stage with done(true); the destructor
     * alone runs on an early error return (HIP_OK), when a launch may have
     * failed and never recorded its events: they go back to the pool unread */
    void done(bool launched = true)
    {
        if (!a)
            return;
        if (launched && rs_launch_timer.n > 0) {
            g.pending.push_back({kernel, a, b});
        } else { /* nothing (successfully) launched */
            g.event_pool.push_back(a);
            g.event_pool.push_back(b);
        }
        rs_launch_timer = {nullptr, nullptr, 0};
        a = b = nullptr;
    }
    ~KernelTimer() { done(false); }
};

/* One stage: the launches of CALL timed under ID on stream S.  A failed launch
 * returns false from the enclosing function, its events back in the pool unread. */
#define STAGE(G, ID, S, CALL)                                                                                         \
    do {                                                                                                              \
        KernelTimer t_((G), (ID), (S));                                                                               \
        HIP_OK(CALL);                                                                                                 \
        t_.done();                                                                                                    \
    } while (0)

/* Folds the finished stage timings into the totals.  An entry whose events
 * cannot be read is dropped (its events recycled) rather than left queued,
 * so one failed launch cannot wedge every later timing call. */
static bool drain_timing(GpuCtx &g)
{
    bool all = true;
    for (auto &t : g.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            g.total_ms[t.kernel] += ms;
            g.launches[t.kernel] += 1;
        } else {
            all = false;
        }
        g.event_pool.push_back(t.a);
        g.event_pool.push_back(t.b);
    }
    g.pending.clear();
    if (!all) {
        (void)hipGetLastError();
        return fail("a timed kernel's events could not be read (launch failed?); entry dropped");
    }
    return true;
}

EXPORT bool poporon_amd_timing(poporon_t *h, int enable)
{
    if (!h)
        return fail("NULL handle");
    if (!gpu_init(h))
        return false;
    DeviceGuard dg(h->gpu.device);
    GpuCtx &g = h->gpu;
    if (!drain_timing(g))
        return false;
    for (int k = 0; k < NKERN; k++) {
        g.total_ms[k] = 0;
        g.launches[k] = 0;
    }
    g.timing = enable != 0;
    return true;
}

EXPORT bool poporon_amd_timing_read(poporon_t *h, int kernel, double *total_ms, uint64_t *launches)
{
    if (!h || kernel < 0 || kernel >= NKERN)
        return fail("bad handle or kernel id");
    if (!h->gpu.ready)
        return fail("no GPU work recorded");
    DeviceGuard dg(h->gpu.device);
    if (!drain_timing(h->gpu))
        return false;
    if (total_ms)
        *total_ms = h->gpu.total_ms[kernel];
    if (launches)
        *launches = h->gpu.launches[kernel];
    return true;
}

/* ------------------------------------------------------------------------ */
/* device batches                                                           */
/* ------------------------------------------------------------------------ */

/* The handle's syndrome workspace (rem) is written and read by launches on
 * whatever stream a call names.  Before a call overwrites it, its stream waits
 * for the last launch that read it if that ran on another stream (same stream:
 * already ordered); after its own last reader the call records rem_done. */
static bool rem_acquire(GpuCtx &g, hipStream_t s)
{
    if (g.rem_pending && g.rem_stream != s)
        HIP_OK(hipStreamWaitEvent(s, g.rem_done, 0));
    return true;
}

static bool rem_release(GpuCtx &g, hipStream_t s)
{
    HIP_OK(hipEventRecord(g.rem_done, s));
    g.rem_stream = s;
    g.rem_pending = true;
    return true;
}

/* general parameters: one codeword per 8..64 lanes (rsgw_*) or per lane
 * (rsg_*).  The wave kernels take single calls and batches below 16,384
 * codewords of every code, every large decode batch of codes of 15 symbols
 * or more (round 6: 8 / 16 / 32 lanes per codeword for codes of up to 31 /
 * 63 / 127 symbols, branch-free BM; 65,536 codewords of 2^m - 1 = 15 / 31 /
 * 63 / 127: 40 / 39 / 70 / 184 us against 80 / 84 / 213 / 745 us per lane,
 * profiles/r06_general_lat_{wave,lane}.log) and large encode batches of
 * 255-symbol codes; the per-lane kernels large decode batches of 3- and
 * 7-symbol codes (22 us vs 32 at m = 2) and large encode batches of shorter
 * codes with more than 32 roots (codes with up to 32 take the RS(255,223) LFSR
 * kernel, params_lfsr_nr) */
static bool gen_wave(const poporon_t *h, size_t count, bool encode, size_t size)
{
    const uint32_t nn = h->rs->gf->field_size;
    if (size < 1 || size + h->rs->num_roots > nn) /* the wave kernels hold one row of <= nn symbols */
        return false;
    if (h->gen_path)
        return h->gen_path == 2;
    return count < 16384 || (encode ? nn == 255u : nn >= 15u);
}

/* the handle's kernel parameters for rows of `size` message bytes (a shortened
 * code: pad = nn - num_roots - size virtual zeros in front; only decodes read it) */
static RsCorrParams corr_params(const poporon_t *h, size_t size)
{
    RsCorrParams prm = h->corr;
    prm.size = (uint32_t)size;
    prm.pad = (int32_t)(h->rs->gf->field_size - h->rs->num_roots - size);
    return prm;
}

static RsGenParams gen_params(const poporon_t *h, size_t size)
{
    RsGenParams prm = h->gen;
    prm.size = (uint32_t)size;
    prm.pad = (int32_t)(h->rs->gf->field_size - h->rs->num_roots - size);
    return prm;
}

#define GEN_LFSR_MIN 1024 /* batch size from which codes of more than 32 roots encode on rsg_lfsr_k */

static bool launch_encode(poporon_t *h, const uint8_t *d_data, size_t ds, uint8_t *d_par, size_t ps, size_t size,
                          size_t count, hipStream_t s)
{
    KernelTimer t(h->gpu, POPORON_AMD_KERNEL_ENCODE, s);
    if (h->fec_type == PPLN_FEC_BCH) {
        HIP_OK(bchk_encode(&h->bch, d_data, ds, d_par, ps, count, h->gpu.num_cu, s));
    } else if (h->fast && count == 1 && size <= 223) { /* one codeword: 223 dependent LFSR steps are the latency */
        HIP_OK(rsk_encode1(h->gpu.tab, d_data, d_par, (uint32_t)size, nullptr, 0, s));
    } else if (h->fast) {
        HIP_OK(rsk_encode(h->gpu.tab, d_data, ds, d_par, ps, (uint32_t)size, count, h->gpu.num_cu, s));
    } else if (h->nrsplit && count == 1 && size <= 255u - h->rs->num_roots) {
        /* one codeword: the whole workgroup (rs_enc1_k reads exp2 / log, which
         * build_decode_tables fills only for nrsplit codes) */
        HIP_OK(rsk_encode1_nr(h->gpu.tab, d_data, d_par, (uint32_t)size, h->rs->num_roots, nullptr, 0u, s));
    } else if (h->lfsr_nr && !h->gen_path) { /* (POPORON_AMD_GENERIC forces the general kernels, as for decode) */
        HIP_OK(rsk_encode_nr(h->gpu.tab, d_data, ds, d_par, ps, (uint32_t)size, count, h->rs->num_roots,
                             h->gpu.num_cu, s));
    } else if (h->rs->num_roots > RS_NR && !h->gen_path && count >= GEN_LFSR_MIN) {
        /* the per-lane LFSR of 16 ceil(nr / 16) bytes (rsg_lfsr_k; smaller
         * batches on the wave kernel, whose codeword spreads over the wave:
         * 64 codewords 27-34 vs 34-41 us, 4,096 39-53 vs 51-53 -> 39-45,
         * 65,536 292-524 vs 43-52 us, profiles/r06_general_lat_auto_v2.log) */
        const RsGenParams prm = gen_params(h, size);
        HIP_OK(rsg_lfsr_encode(h->gpu.gtab, &prm, d_data, ds, d_par, ps, count, h->gpu.num_cu, s));
    } else {
        const RsGenParams prm = gen_params(h, size);
        if (gen_wave(h, count, true, size))
            HIP_OK(rsgw_encode(h->gpu.gtab, &prm, d_data, ds, d_par, ps, count, nullptr, 0u, h->gpu.num_cu, s));
        else
            HIP_OK(rsg_encode(h->gpu.gtab, &prm, d_data, ds, d_par, ps, count, h->gpu.num_cu, s));
    }
    t.done();
    return true;
}

/* batches from this size on take the split kernels (rs_fast.hip, six
 * launches, one codeword per lane); smaller ones one launch of rs_wave_k (one
 * codeword per wave).  Where they cross (16 errors, wall time per call,
 * profiles/r04_batchlat_*.log): 12,288 codewords 86 vs ~108 us, 16,384 107 vs
 * ~108, 32,768 196 vs ~110 */
#define SPLIT_MIN_COUNT 16384

/* One batch decode, as every entry point describes it (device pointers) */
struct DecodeCall {
    uint8_t *data;
    size_t ds;
    uint8_t *par;
    size_t ps;
    size_t size, count;
    const uint16_t *ext_syn; /* external log-form syndromes (src/decode.c:446-464); NULL: the rows' own */
    size_t ext_stride;
    const uint8_t *pos8; /* erasure slots as u8 or as u32 (never both; neither: errors only), */
    const uint32_t *pos32;
    size_t pos_stride;  /* pos_stride elements apart, */
    const uint8_t *cnt; /* and how many of each row's slots count */
    uint8_t *ok, *corrected;
    hipStream_t s;
    uint8_t *rem; /* the caller's workspace of rs_ws_bytes(rem_cap) bytes, rem_cap >= count; NULL: the handle's */
    size_t rem_cap;
};

enum DecodeRoute {
    ROUTE_BCH,        /* bchk_decode */
    ROUTE_SINGLE,     /* one codeword on one workgroup (rsk_decode1): 32 roots or fewer, every mode */
    ROUTE_GENERAL,    /* general parameters: one codeword per wave or per lane (rsgw_decode / rsg_decode) */
    ROUTE_WAVE,       /* one codeword per wave, syndromes included, one launch (rsk_wave) */
    ROUTE_SPLIT,      /* errors only, the rows' syndromes or external ones: the split kernels (launch_split) */
    ROUTE_ERRATA,     /* u8 erasure slots in 4-byte aligned rows: the errata kernels (launch_errata) */
    ROUTE_ERA_ERRATA, /* ... in 16-byte aligned rows, prim 1: rsk_era first, the errata kernels for what it leaves */
    ROUTE_ERA,        /* ... rsk_era alone (rows the errata kernels cannot read) */
    ROUTE_ERA_RECORD, /* any other erasure slots: rsk_correct_era_rec, its records applied block-wise */
    ROUTE_CORRECT     /* the rest: the single kernel over the whole batch (rsk_correct) */
};

/* Does the batch take the lane-per-codeword kernels (rs_fast.hip, rs_errata.hip)?
 * RS(255,223): from SPLIT_MIN_COUNT codewords on.  A byte-symbol code of fewer
 * than 32 roots: at every batch size, single calls included -- the general
 * kernel's one lane per codeword takes ~1 ms whatever the count, the six split
 * launches ~0.1 ms from 1 to 65,536 codewords of RS(255,239)
 * (profiles/r05_nr_batchlat.log). */
static bool split_ok(const poporon_t *h, size_t count)
{
    if (!h->corr.vfast || h->corr.force_verify)
        return false;
    if (h->nrsplit)
        return h->decode_path == 0 || h->decode_path == 1;
    return h->decode_path != 2 && (h->decode_path == 1 || count >= SPLIT_MIN_COUNT);
}

/* Which kernels decode the call: decided here and nowhere else, from the
 * handle and the call alone (no HIP call, no side effect).  The order of the
 * tests is the dispatch. */
static DecodeRoute decode_route(const poporon_t *h, const DecodeCall &c)
{
    if (h->fec_type == PPLN_FEC_BCH)
        return ROUTE_BCH;
    const bool era = c.pos8 || c.pos32;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(c.pos8);
    /* u8 slots in rows the errata kernels read word by word */
    const bool rows4 = c.pos8 && c.pos_stride >= h->rs->num_roots && c.pos_stride % 4u == 0u && (pa & 3u) == 0u;
    if (h->nrsplit) {
        if (c.count == 1 && h->decode_path == 0)
            return ROUTE_SINGLE;
        if (!era && split_ok(h, c.count))
            return ROUTE_SPLIT;
        if (rows4 && !c.ext_syn && split_ok(h, c.count))
            return ROUTE_ERRATA;
    }
    if (!h->fast)
        return ROUTE_GENERAL;
    if (c.count == 1)
        return ROUTE_SINGLE;
    /* a few thousand codewords: the lane-per-codeword kernels would give each
     * SIMD a few waves, each a ~10^4-step serial chain */
    if (h->decode_path == 3 || (h->decode_path == 0 && c.count < SPLIT_MIN_COUNT))
        return ROUTE_WAVE;
    if (!split_ok(h, c.count))
        return ROUTE_CORRECT;
    if (!era)
        return ROUTE_SPLIT;
    if (c.ext_syn)
        return ROUTE_CORRECT;
    /* u8 slots: rs_era_bp_k for 32 sorted erasures (prim 1, rows read as
     * uint4), the errata kernels for every other count with or without errors;
     * u32 slots and unaligned rows: the record kernel for all */
    if (c.pos8 && h->corr.prim == 1u && c.pos_stride % 16u == 0u && (pa & 15u) == 0u)
        return rows4 ? ROUTE_ERA_ERRATA : ROUTE_ERA;
    return rows4 ? ROUTE_ERRATA : ROUTE_ERA_RECORD;
}

/* The workspace of one call: the caller's if it brought one, else the handle's
 * (grown to the count and ordered behind its last reader on another stream).
 * ws_release after the call's last reader -- never on an error return, which
 * leaves rem_done unrecorded. */
struct DecodeWs {
    uint8_t *rem = nullptr;
    bool shared = false;
    RsSplitWs ws = {};
};

static bool ws_acquire(poporon_t *h, uint8_t *rem, size_t rem_cap, size_t count, hipStream_t s, DecodeWs &w)
{
    w.shared = !rem;
    if (w.shared) {
        if (!ensure_rem(h, count) || !rem_acquire(h->gpu, s))
            return false;
        rem = h->gpu.rem;
        rem_cap = h->gpu.rem_cap;
    }
    w.rem = rem;
    w.ws = rs_ws_carve(rem, rem_cap ? rem_cap : count);
    return true;
}

static bool ws_release(poporon_t *h, const DecodeWs &w, hipStream_t s) { return !w.shared || rem_release(h->gpu, s); }

/* what the lane-per-codeword kernels of a fewer-roots code hand on (ws.list):
 * the general kernel, per lane or per wave, in the call's own mode */
static hipError_t launch_list_nr(poporon_t *h, const DecodeCall &c, const RsSplitWs &ws)
{
    GpuCtx &g = h->gpu;
    const RsGenParams gp = gen_params(h, c.size);
    const size_t xs = c.ext_syn ? c.ext_stride : 0, es = c.pos8 ? c.pos_stride : 0;
    const uint8_t *cnt = c.pos8 ? c.cnt : nullptr;
    if (h->gen_path == 1)
        return rsg_decode_list(g.gtab, &gp, c.data, c.ds, c.par, c.ps, c.count, ws.list, ws.nlist, c.ext_syn, xs,
                               c.pos8, es, cnt, c.ok, c.corrected, g.num_cu, c.s);
    return rsgw_decode(g.gtab, &gp, c.data, c.ds, c.par, c.ps, c.count, c.ext_syn, xs, c.pos8, nullptr, es, cnt, c.ok,
                       c.corrected, ws.list, ws.nlist, nullptr, 0u, g.num_cu, c.s);
}

/* How the split decode ends (decode_tail).  Left to the count, rs_search_apply_k takes the batches that
 * give its one workgroup per CU more than one 1024-row batch, the ones whose waves have a next batch to
 * search while a block's rows are in flight: 0.130 against 0.171 ms at 2^20 rows.  Smaller batches keep
 * rs_chien_k and rs_forney_apply_k, the launches that the recorded route table
 * (tests/golden/decode_routes.json) names for them; the one kernel measured 4-5 us shorter there as well
 * (33 against 38 us at 16,384 rows, profiles/search_tail_counts.log), a gain left for a change that
 * records the table anew.  POPORON_AMD_DECODE_TAIL=search takes it at every count. */
static int split_tail(const poporon_t *h, size_t count)
{
    if (h->decode_tail != 3)
        return h->decode_tail;
    const size_t cus = (size_t)(h->gpu.num_cu > 0 ? h->gpu.num_cu : 256);
    return count > cus * 1024u ? 2 : 0;
}

/* ROUTE_SPLIT: the split error-mode decode (rs_fast.hip, one codeword per
 * lane; what it hands on: one codeword per wave); fewer than 32 roots: the
 * _nr kernels, the list on the general kernel */
static bool launch_split(poporon_t *h, const DecodeCall &c)
{
    GpuCtx &g = h->gpu;
    hipStream_t s = c.s;
    const uint32_t npar = h->rs->num_roots, size = (uint32_t)c.size;
    const bool nr = npar < RS_NR;
    const RsCorrParams prm = corr_params(h, c.size);
    DecodeWs w;
    if (!ws_acquire(h, c.rem, c.rem_cap, c.count, s, w))
        return false;
    const RsSplitWs &ws = w.ws;
    /* (external syndromes: converted, refusals to the list) */
    STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
          c.ext_syn ? rsk_ext_syn(g.tab, c.ext_syn, c.ext_stride, c.count, npar, ws.syn, ws.list, ws.nlist, s)
          : nr      ? rsk_syndrome_reset_nr(g.tab, c.data, c.ds, c.par, c.ps, size, c.count, ws.syn, ws.nlist, npar,
                                            g.num_cu, s)
                    : rsk_syndrome_reset(g.tab, c.data, c.ds, c.par, c.ps, size, c.count, ws.syn, ws.nlist, g.num_cu,
                                         s));
    STAGE(g, POPORON_AMD_KERNEL_BM, s,
          nr ? rsk_bm_nr(g.tab, &ws, c.count, npar, c.ok, c.corrected, g.num_cu, s)
             : rsk_bm(g.tab, &ws, c.count, c.ok, c.corrected, g.num_cu, s));
    const int tail = split_tail(h, c.count);
    if (tail != 2)
        STAGE(g, POPORON_AMD_KERNEL_CHIEN, s, rsk_chien(g.tab, &prm, &ws, c.count, c.ok, c.corrected, g.num_cu, s));
    if (tail == 2) {
        /* the root search too (rs_search_apply_k), charged to the apply's id: the Chien id records no launch */
        STAGE(g, POPORON_AMD_KERNEL_APPLY, s,
              rsk_search_apply(g.tab, &prm, &ws, c.data, c.ds, c.par, c.ps, c.count, npar, c.ok, c.corrected, g.num_cu,
                               s));
    } else if (tail == 0) {
        /* Forney and the block apply in one kernel (rs_forney_apply_k), charged to the apply's id */
        STAGE(g, POPORON_AMD_KERNEL_APPLY, s,
              rsk_forney_apply(g.tab, &prm, &ws, c.data, c.ds, c.par, c.ps, c.count, npar, c.ok, c.corrected, g.num_cu,
                               s));
    } else {
        STAGE(g, POPORON_AMD_KERNEL_FORNEY, s,
              rsk_forney(g.tab, &prm, &ws, c.data, c.ds, c.par, c.ps, c.count, c.ok, c.corrected, g.num_cu, s));
        STAGE(g, POPORON_AMD_KERNEL_APPLY, s,
              nr ? rsk_apply_nr(&prm, &ws, c.data, c.ds, c.par, c.ps, c.count, npar, s)
                 : rsk_apply(&prm, &ws, c.data, c.ds, c.par, c.ps, c.count, s));
    }
    STAGE(g, POPORON_AMD_KERNEL_LIST, s,
          nr ? launch_list_nr(h, c, ws)
             : rsk_wave(g.tab, &prm, c.data, c.ds, c.par, c.ps, c.count, ws.list, ws.nlist,
                        c.ext_syn ? nullptr : ws.syn, c.ext_syn, c.ext_syn ? c.ext_stride : 0, nullptr, nullptr, 0,
                        nullptr, c.ok, c.corrected, g.num_cu, s));
    return ws_release(h, w, s);
}

/* ROUTE_ERRATA / ROUTE_ERA_ERRATA / ROUTE_ERA: erasure batches in u8 slots.
 * Records (64 B per codeword in ws.ext) applied block-wise: scattered byte
 * read-modify-writes cost ~0.3 ms per 2^20 codewords with 32 erasures.  What
 * the kernels hand on stays RS_ST_LIST in ws.meta: decoded in place by the
 * list kernel, passed by in the record apply.  Fewer than 32 roots: the _nr
 * kernels (never rsk_era), the list on the general kernel in erasure mode. */
static bool launch_errata(poporon_t *h, const DecodeCall &c, bool era_first, bool errata)
{
    GpuCtx &g = h->gpu;
    hipStream_t s = c.s;
    const uint32_t npar = h->rs->num_roots, size = (uint32_t)c.size;
    const bool nr = npar < RS_NR;
    const uint32_t only_pend = era_first ? 1u : 0u; /* the errata kernels take what rsk_era left pending */
    const RsCorrParams prm = corr_params(h, c.size);
    DecodeWs w;
    if (!ws_acquire(h, c.rem, c.rem_cap, c.count, s, w))
        return false;
    const RsSplitWs &ws = w.ws;
    STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
          nr ? rsk_syndrome_reset_nr(g.tab, c.data, c.ds, c.par, c.ps, size, c.count, ws.syn, ws.nlist, npar, g.num_cu,
                                     s)
             : rsk_syndrome_reset(g.tab, c.data, c.ds, c.par, c.ps, size, c.count, ws.syn, ws.nlist, g.num_cu, s));
    if (era_first)
        STAGE(g, POPORON_AMD_KERNEL_ERASURE, s,
              rsk_era(g.tab, &prm, &ws, c.pos8, c.pos_stride, c.cnt, c.count, c.ok, c.corrected, errata ? 1u : 0u,
                      g.num_cu, s));
    if (errata) {
        STAGE(g, POPORON_AMD_KERNEL_BM, s,
              nr ? rsk_ebm_nr(g.tab, &prm, &ws, c.pos8, c.pos_stride, c.cnt, c.count, c.ok, c.corrected, npar,
                              g.num_cu, s)
                 : rsk_ebm(g.tab, &prm, &ws, c.pos8, c.pos_stride, c.cnt, c.count, c.ok, c.corrected, only_pend,
                           g.num_cu, s));
        STAGE(g, POPORON_AMD_KERNEL_CHIEN, s,
              rsk_chien32(g.tab, &prm, &ws, c.count, c.ok, c.corrected, only_pend, g.num_cu, s));
        STAGE(g, POPORON_AMD_KERNEL_FORNEY, s,
              nr ? rsk_forney32_nr(g.tab, &prm, &ws, c.pos8, c.pos_stride, c.count, c.ok, c.corrected, npar, g.num_cu,
                                   s)
                 : rsk_forney32(g.tab, &prm, &ws, c.pos8, c.pos_stride, c.count, c.ok, c.corrected, only_pend,
                                g.num_cu, s));
    }
    STAGE(g, POPORON_AMD_KERNEL_LIST, s,
          nr ? launch_list_nr(h, c, ws)
             : rsk_wave(g.tab, &prm, c.data, c.ds, c.par, c.ps, c.count, ws.list, ws.nlist, ws.syn, nullptr, 0, c.pos8,
                        nullptr, c.pos_stride, c.cnt, c.ok, c.corrected, g.num_cu, s));
    STAGE(g, POPORON_AMD_KERNEL_APPLY, s,
          nr ? rsk_apply_era_nr(&prm, ws.meta, ws.ext, c.data, c.ds, c.par, c.ps, c.count, npar, s)
             : rsk_apply_era(&prm, ws.meta, ws.ext, c.data, c.ds, c.par, c.ps, c.count, s));
    return ws_release(h, w, s);
}

/* ROUTE_ERA_RECORD: u32 slots and u8 slots in unaligned rows */
static bool launch_era_record(poporon_t *h, const DecodeCall &c)
{
    GpuCtx &g = h->gpu;
    hipStream_t s = c.s;
    const RsCorrParams prm = corr_params(h, c.size);
    DecodeWs w;
    if (!ws_acquire(h, c.rem, c.rem_cap, c.count, s, w))
        return false;
    const RsSplitWs &ws = w.ws;
    STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
          rsk_syndrome(g.tab, c.data, c.ds, c.par, c.ps, (uint32_t)c.size, c.count, ws.syn, g.num_cu, s));
    STAGE(g, POPORON_AMD_KERNEL_CORRECT, s,
          rsk_correct_era_rec(g.tab, &prm, c.count, ws.syn, c.pos8, c.pos32, c.pos_stride, c.cnt, c.ok, c.corrected,
                              ws.ext, ws.meta, g.num_cu, s));
    STAGE(g, POPORON_AMD_KERNEL_APPLY, s,
          rsk_apply_era(&prm, ws.meta, ws.ext, c.data, c.ds, c.par, c.ps, c.count, s));
    return ws_release(h, w, s);
}

/* ROUTE_CORRECT: syndromes, then the whole decode in one kernel */
static bool launch_correct(poporon_t *h, const DecodeCall &c)
{
    GpuCtx &g = h->gpu;
    hipStream_t s = c.s;
    const RsCorrParams prm = corr_params(h, c.size);
    DecodeWs w;
    /* external syndromes and no caller workspace: none at all (rsk_correct reads c.ext_syn, never rem) */
    if ((c.rem || !c.ext_syn) && !ws_acquire(h, c.rem, c.rem_cap, c.count, s, w))
        return false;
    if (!c.ext_syn)
        STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
              rsk_syndrome(g.tab, c.data, c.ds, c.par, c.ps, (uint32_t)c.size, c.count, w.rem, g.num_cu, s));
    STAGE(g, POPORON_AMD_KERNEL_CORRECT, s,
          rsk_correct(g.tab, &prm, c.data, c.ds, c.par, c.ps, c.count, w.rem, c.ext_syn, c.ext_stride, c.pos8, c.pos32,
                      c.pos_stride, c.cnt, c.ok, c.corrected, g.num_cu, s));
    return ws_release(h, w, s);
}

/* One batch decode on the device: the route, then its launcher */
static bool launch_decode(poporon_t *h, const DecodeCall &c)
{
    GpuCtx &g = h->gpu;
    hipStream_t s = c.s;
    /* rsk_decode1's mode: 0 errors, 1 erasure slots, 2 external syndromes */
    const uint32_t mode1 = c.ext_syn ? 2u : (c.pos8 || c.pos32) ? 1u : 0u;
    switch (decode_route(h, c)) {
    case ROUTE_BCH:
        if (c.ext_syn || c.pos8 || c.pos32)
            return fail("BCH has no erasure or external-syndrome decode");
        STAGE(g, POPORON_AMD_KERNEL_CORRECT, s,
              bchk_decode(&h->bch, c.data, c.ds, c.par, c.ps, c.count, c.ok, c.corrected, g.num_cu, s));
        return true;
    case ROUTE_SINGLE: { /* (rs_single.hip; P.nr = num_roots; it always runs the check) */
        const RsCorrParams prm = corr_params(h, c.size);
        STAGE(g, POPORON_AMD_KERNEL_SINGLE, s,
              rsk_decode1(g.tab, &prm, mode1, c.data, c.par, c.pos8, c.pos32, c.cnt, 1u, c.ext_syn, c.ok, c.corrected,
                          nullptr, 0, s));
        return true;
    }
    case ROUTE_GENERAL: {
        const RsGenParams prm = gen_params(h, c.size);
        STAGE(g, POPORON_AMD_KERNEL_CORRECT, s,
              gen_wave(h, c.count, false, c.size)
                  ? rsgw_decode(g.gtab, &prm, c.data, c.ds, c.par, c.ps, c.count, c.ext_syn, c.ext_stride, c.pos8,
                                c.pos32, c.pos_stride, c.cnt, c.ok, c.corrected, nullptr, nullptr, nullptr, 0u,
                                g.num_cu, s)
                  : rsg_decode(g.gtab, &prm, c.data, c.ds, c.par, c.ps, c.count, c.ext_syn, c.ext_stride, c.pos8,
                               c.pos32, c.pos_stride, c.cnt, c.ok, c.corrected, g.num_cu, s));
        return true;
    }
    case ROUTE_WAVE: {
        const RsCorrParams prm = corr_params(h, c.size);
        STAGE(g, POPORON_AMD_KERNEL_WAVE, s,
              rsk_wave(g.tab, &prm, c.data, c.ds, c.par, c.ps, c.count, nullptr, nullptr, nullptr, c.ext_syn,
                       c.ext_stride, c.pos8, c.pos32, c.pos_stride, c.cnt, c.ok, c.corrected, g.num_cu, s));
        return true;
    }
    case ROUTE_SPLIT:
        return launch_split(h, c);
    case ROUTE_ERRATA:
        return launch_errata(h, c, false, true);
    case ROUTE_ERA_ERRATA:
        return launch_errata(h, c, true, true);
    case ROUTE_ERA:
        return launch_errata(h, c, true, false);
    case ROUTE_ERA_RECORD:
        return launch_era_record(h, c);
    case ROUTE_CORRECT:
        return launch_correct(h, c);
    }
    return false; /* (every route returns above) */
}

/* d_dirty[c] = codeword c's syndrome is nonzero (RS handles) */
static bool launch_check(poporon_t *h, const uint8_t *d_data, size_t data_stride, const uint8_t *d_parity,
                         size_t parity_stride, size_t size, size_t count, uint8_t *d_dirty, hipStream_t s)
{
    KernelTimer t(h->gpu, POPORON_AMD_KERNEL_CHECK, s);
    if (h->fast) {
        HIP_OK(rsk_check(h->gpu.tab, d_data, data_stride, d_parity, parity_stride, (uint32_t)size, count, d_dirty,
                         h->gpu.num_cu, s));
    } else if (h->nrsplit) {
        HIP_OK(rsk_check_nr(h->gpu.tab, d_data, data_stride, d_parity, parity_stride, (uint32_t)size, count, d_dirty,
                            h->rs->num_roots, h->gpu.num_cu, s));
    } else {
        const RsGenParams prm = gen_params(h, size);
        if (gen_wave(h, count, false, size))
            HIP_OK(rsgw_check(h->gpu.gtab, &prm, d_data, data_stride, d_parity, parity_stride, count, d_dirty,
                              nullptr, 0, h->gpu.num_cu, s));
        else
            HIP_OK(rsg_check(h->gpu.gtab, &prm, d_data, data_stride, d_parity, parity_stride, count, d_dirty,
                             nullptr, 0, h->gpu.num_cu, s));
    }
    t.done();
    return true;
}

EXPORT bool poporon_check_batch_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                       const uint8_t *d_parity, size_t parity_stride, size_t size, size_t count,
                                       uint8_t *d_dirty, void *stream)
{
    if (!h || (count && (!d_data || !d_parity || !d_dirty)))
        return fail("NULL argument");
    if (h->fec_type != PPLN_FEC_RS)
        return fail("poporon_check_batch_device serves RS handles");
    if (!check_decode_size(h, size))
        return fail("size %zu outside [1, %u]", size, (unsigned)kmax(h));
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    DeviceGuard dg(h->gpu.device);
    return launch_check(h, d_data, data_stride, d_parity, parity_stride, size, count, d_dirty, (hipStream_t)stream);
}

EXPORT bool poporon_syndrome_batch_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                          const uint8_t *d_parity, size_t parity_stride, size_t size, size_t count,
                                          uint16_t *d_syndromes, size_t syndrome_stride, uint8_t *d_nonzero,
                                          void *stream)
{
    if (!h || (count && (!d_data || !d_parity || (!d_syndromes && !d_nonzero))))
        return fail("NULL argument");
    if (h->fec_type != PPLN_FEC_RS)
        return fail("poporon_syndrome_batch_device serves RS handles");
    if (d_syndromes && syndrome_stride < h->rs->num_roots)
        return fail("syndrome_stride < num_roots (%u)", (unsigned)h->rs->num_roots);
    if (!check_decode_size(h, size))
        return fail("size %zu outside [1, %u]", size, (unsigned)kmax(h));
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    DeviceGuard dg(h->gpu.device);
    hipStream_t s = (hipStream_t)stream;
    GpuCtx &g = h->gpu;
    const uint32_t nr = h->rs->num_roots;
    if (!h->fast && !h->nrsplit) {
        const RsGenParams prm = gen_params(h, size);
        STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
              gen_wave(h, count, false, size)
                  ? rsgw_check(g.gtab, &prm, d_data, data_stride, d_parity, parity_stride, count, d_nonzero,
                               d_syndromes, syndrome_stride, g.num_cu, s)
                  : rsg_check(g.gtab, &prm, d_data, data_stride, d_parity, parity_stride, count, d_nonzero, d_syndromes,
                              syndrome_stride, g.num_cu, s));
        return true;
    }
    /* the LFSR kernel's syndromes into the handle's workspace (fewer roots: npar of them), then their logs */
    DecodeWs w;
    if (!ws_acquire(h, nullptr, 0, count, s, w))
        return false;
    STAGE(g, POPORON_AMD_KERNEL_REMAINDER, s,
          h->nrsplit ? rsk_syndrome_reset_nr(g.tab, d_data, data_stride, d_parity, parity_stride, (uint32_t)size, count,
                                             w.rem, nullptr, nr, g.num_cu, s)
                     : rsk_syndrome(g.tab, d_data, data_stride, d_parity, parity_stride, (uint32_t)size, count, w.rem,
                                    g.num_cu, s));
    HIP_OK(h->nrsplit ? rsk_syn_log_nr(g.tab, w.rem, count, d_syndromes, syndrome_stride, d_nonzero, nr, s)
                      : rsk_syn_log(g.tab, w.rem, count, d_syndromes, syndrome_stride, d_nonzero, s));
    return ws_release(h, w, s);
}

EXPORT bool poporon_encode_batch_device(poporon_t *h, const uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                        size_t parity_stride, size_t size, size_t count, void *stream)
{
    if (!h || (count && (!d_data || !d_parity)))
        return fail("NULL argument");
    if (is_ldpc(h, "poporon_encode_batch_device"))
        return false;
    if (!check_encode_size(h, size))
        return false;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    DeviceGuard dg(h->gpu.device);
    return launch_encode(h, d_data, data_stride, d_parity, parity_stride, size, count, (hipStream_t)stream);
}

EXPORT bool poporon_decode_batch_device(poporon_t *h, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                        size_t parity_stride, size_t size, size_t count, const uint8_t *d_positions,
                                        size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                        uint8_t *d_corrected, void *stream)
{
    if (!decode_row_args(h, "poporon_decode_batch_device", false, d_data, d_parity, size, count, d_positions,
                         positions_stride, d_counts, d_ok))
        return false;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    DeviceGuard dg(h->gpu.device);
    return launch_decode(h, {.data = d_data, .ds = data_stride, .par = d_parity, .ps = parity_stride, .size = size,
                             .count = count, .pos8 = d_positions, .pos_stride = positions_stride, .cnt = d_counts,
                             .ok = d_ok, .corrected = d_corrected, .s = (hipStream_t)stream});
}

EXPORT bool poporon_decode_batch_syndrome_device(poporon_t *h, uint8_t *d_data, size_t data_stride,
                                                 uint8_t *d_parity, size_t parity_stride, size_t size, size_t count,
                                                 const uint16_t *d_syndromes, size_t syndrome_stride, uint8_t *d_ok,
                                                 uint8_t *d_corrected, void *stream)
{
    if (!h || (count && (!d_data || !d_parity || !d_ok || !d_syndromes)))
        return fail("NULL argument");
    if (h->fec_type != PPLN_FEC_RS)
        return fail("external-syndrome decode serves RS handles");
    if (syndrome_stride < h->rs->num_roots)
        return fail("syndrome_stride < num_roots (%u)", (unsigned)h->rs->num_roots);
    if (!check_decode_size(h, size))
        return fail("decode size %zu outside [1, %u]", size, (unsigned)kmax(h));
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    DeviceGuard dg(h->gpu.device);
    return launch_decode(h, {.data = d_data, .ds = data_stride, .par = d_parity, .ps = parity_stride, .size = size,
                             .count = count, .ext_syn = d_syndromes, .ext_stride = syndrome_stride, .ok = d_ok,
                             .corrected = d_corrected, .s = (hipStream_t)stream});
}

/* ------------------------------------------------------------------------ */
/* host batches: staged through device memory in chunks                     */
/* ------------------------------------------------------------------------ */

/*
 * Host batches are streamed through PIPE_SLOTS slots, each with its own HIP
 * stream, pinned host buffer and device buffer.  Chunk i goes to slot
 * i % PIPE_SLOTS: its rows are gathered into pinned memory (CPU threads),
 * copied in, processed and copied back asynchronously; the slot's results are
 * scattered to the caller's arrays only when the slot is needed again (or at
 * the end).  So the CPU gather of chunk i+1, the H2D copy of chunk i+1, the
 * kernels of chunk i and the D2H copy of chunk i-1 overlap.
 */
static const size_t kPipeChunk = 1u << 18; /* codewords per chunk */

/* row copy dst[c*dw .. +w) = src[c*sw .. +w) for c < count, split over CPU threads */
static void copy_rows(uint8_t *dst, size_t dw, const uint8_t *src, size_t sw, size_t w, size_t count)
{
    auto run = [=](size_t a, size_t b) {
        if (dw == w && sw == w) {
            memcpy(dst + a * w, src + a * w, (b - a) * w);
            return;
        }
        for (size_t c = a; c < b; c++)
            memcpy(dst + c * dw, src + c * sw, w);
    };
    const size_t bytes = w * count;
    unsigned nt = std::thread::hardware_concurrency();
    nt = std::max(1u, std::min(nt, 16u));
    if (bytes < (4u << 20) || nt == 1) {
        run(0, count);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = (count + nt - 1) / nt;
    for (unsigned t = 1; t < nt; t++) {
        const size_t a = std::min(count, t * per), b = std::min(count, a + per);
        if (a < b)
            th.emplace_back(run, a, b);
    }
    run(0, std::min(count, per));
    for (auto &x : th)
        x.join();
}

static bool pipe_slot(poporon_t *h, GpuCtx::PipeSlot &ps, size_t bytes)
{
    if (!ps.stream)
        HIP_OK(hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking));
    if (!ps.done)
        HIP_OK(hipEventCreateWithFlags(&ps.done, hipEventDisableTiming));
    if (ps.cap >= bytes)
        return true;
    HIP_OK(hipStreamSynchronize(ps.stream));
    (void)hipHostFree(ps.host);
    (void)hipFree(ps.dev);
    ps.host = nullptr;
    ps.dev = nullptr;
    ps.cap = 0;
    HIP_OK(hipHostMalloc((void **)&ps.host, bytes, hipHostMallocDefault));
    HIP_OK(hipMalloc((void **)&ps.dev, bytes));
    ps.cap = bytes;
    return true;
}

/*
 * The one loop of every host-memory batch: `count` rows in chunks of `chunk`
 * through `nslots` slots of at least slot_bytes each.  Chunk i goes to slot
 * i % nslots: in(host, c0, n) packs rows [c0, c0 + n) into the slot's pinned
 * buffer, run(slot, n) copies in, launches and copies back on the slot's
 * stream, and out(host, c0, n) hands the results to the caller's arrays once
 * the slot's event has fired -- when the slot is needed again, or oldest first
 * after the last chunk.  One slot: a synchronous loop.  After a failure every
 * slot's stream is synchronised before the call returns (nothing may still be
 * in flight into the pinned buffers) and the error text saved by whatever
 * failed is raised again, `what` if nothing saved one.
 */
template <typename In, typename Run, typename Out>
static bool host_chunks(poporon_t *h, GpuCtx::PipeSlot *slots, size_t nslots, size_t count, size_t chunk,
                        size_t slot_bytes, In in, Run run, Out out, const char *what)
{
    for (size_t k = 0; k < nslots; k++)
        if (!pipe_slot(h, slots[k], slot_bytes))
            return false;
    auto finish = [&](GpuCtx::PipeSlot &ps) -> bool {
        if (!ps.busy)
            return true;
        ps.busy = false;
        HIP_OK(hipEventSynchronize(ps.done));
        out(ps.host, ps.c0, ps.n);
        return true;
    };
    bool good = true;
    size_t i = 0;
    for (size_t c0 = 0; good && c0 < count; c0 += chunk, i++) {
        GpuCtx::PipeSlot &ps = slots[i % nslots];
        if (!(good = finish(ps)))
            break;
        const size_t n = std::min(chunk, count - c0);
        in(ps.host, c0, n);
        good = run(ps, n) && hipEventRecord(ps.done, ps.stream) == hipSuccess;
        ps.busy = true;
        ps.c0 = c0;
        ps.n = n;
    }
    for (size_t k = 0; good && k < nslots; k++) /* oldest first */
        good = finish(slots[(i + k) % nslots]);
    if (!good) {
        const std::string msg = g_last_error.empty() ? std::string(what) : g_last_error;
        for (size_t k = 0; k < nslots; k++) {
            if (slots[k].stream)
                (void)hipStreamSynchronize(slots[k].stream);
            slots[k].busy = false;
        }
        return fail("%s", msg.c_str());
    }
    return true;
}

EXPORT bool poporon_encode_batch(poporon_t *h, const uint8_t *data, size_t data_stride, uint8_t *parity,
                                 size_t parity_stride, size_t size, size_t count)
{
    if (!h || (count && (!data || !parity)))
        return fail("NULL argument");
    if (is_ldpc(h, "poporon_encode_batch"))
        return false;
    if (!check_encode_size(h, size))
        return false;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    DeviceGuard dg(h->gpu.device);
    const size_t nr = par_bytes(h);
    const size_t chunk = std::max<size_t>(1, std::min(count, kPipeChunk));
    /* slot layout for n rows: [data size n | parity nr n] */
    return host_chunks(
        h, h->gpu.pipe, PIPE_SLOTS, count, chunk, chunk * (size + nr) + 64,
        [&](uint8_t *hb, size_t c0, size_t n) { copy_rows(hb, size, data + c0 * data_stride, data_stride, size, n); },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            uint8_t *dp = ps.dev + n * size;
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, n * size, hipMemcpyHostToDevice, ps.stream));
            if (!launch_encode(h, ps.dev, size, dp, nr, size, n, ps.stream))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host + n * size, dp, n * nr, hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) {
            copy_rows(parity + c0 * parity_stride, parity_stride, hb + n * size, nr, nr, n);
        },
        "HIP failure in the host pipeline");
}

EXPORT bool poporon_decode_batch(poporon_t *h, uint8_t *data, size_t data_stride, uint8_t *parity,
                                 size_t parity_stride, size_t size, size_t count, const uint8_t *positions,
                                 size_t positions_stride, const uint8_t *counts, uint8_t *ok, uint8_t *corrected)
{
    if (!decode_row_args(h, "poporon_decode_batch", false, data, parity, size, count, positions, positions_stride,
                         counts, ok))
        return false;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    DeviceGuard dg(h->gpu.device);
    const size_t nr = par_bytes(h);
    const size_t w = size + nr;
    const size_t chunk = std::max<size_t>(1, std::min(count, kPipeChunk));
    const size_t per = w + 2 + (positions ? nr + 1 : 0);
    /* parity right after the data in rows of equal stride (the wire layout): move whole rows */
    const bool rows = parity == data + size && parity_stride == data_stride;
    /* slot layout for n rows: [codewords w n | ok n | cor n | to 16 | positions nr n | counts n | to 256 |
     * decode workspace (device)]; positions 16-byte aligned: the 32-erasure kernel reads them as uint4 */
    auto o_ok = [&](size_t n) { return n * w; };
    auto o_pos = [&](size_t n) { return rs_ws_round16(n * w + 2 * n); };
    auto o_cnt = [&](size_t n) { return o_pos(n) + (positions ? n * nr : 0); };
    auto o_rem = [&](size_t n) { return (o_cnt(n) + (positions ? n : 0) + 255) & ~(size_t)255; };
    return host_chunks(
        h, h->gpu.pipe, PIPE_SLOTS, count, chunk, chunk * per + 512 + rs_ws_bytes(chunk),
        [&](uint8_t *hb, size_t c0, size_t n) {
            if (rows) {
                copy_rows(hb, w, data + c0 * data_stride, data_stride, w, n);
            } else {
                copy_rows(hb, w, data + c0 * data_stride, data_stride, size, n);
                copy_rows(hb + size, w, parity + c0 * parity_stride, parity_stride, nr, n);
            }
            if (positions) {
                copy_rows(hb + o_pos(n), nr, positions + c0 * positions_stride, positions_stride, nr, n);
                memcpy(hb + o_cnt(n), counts + c0, n);
            }
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            uint8_t *dc = ps.dev;
            HIP_OK(hipMemcpyAsync(dc, ps.host, n * w, hipMemcpyHostToDevice, ps.stream));
            if (positions)
                HIP_OK(hipMemcpyAsync(dc + o_pos(n), ps.host + o_pos(n), n * nr + n, hipMemcpyHostToDevice, ps.stream));
            if (!launch_decode(h, {.data = dc, .ds = w, .par = dc + size, .ps = w, .size = size, .count = n,
                                   .pos8 = positions ? dc + o_pos(n) : nullptr, .pos_stride = nr,
                                   .cnt = positions ? dc + o_cnt(n) : nullptr, .ok = dc + o_ok(n),
                                   .corrected = dc + o_ok(n) + n, .s = ps.stream, .rem = dc + o_rem(n), .rem_cap = n}))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host, dc, n * w + 2 * n, hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) {
            if (rows) {
                copy_rows(data + c0 * data_stride, data_stride, hb, w, w, n);
            } else {
                copy_rows(data + c0 * data_stride, data_stride, hb, w, size, n);
                copy_rows(parity + c0 * parity_stride, parity_stride, hb + size, w, nr, n);
            }
            memcpy(ok + c0, hb + o_ok(n), n);
            if (corrected)
                memcpy(corrected + c0, hb + o_ok(n) + n, n);
        },
        "HIP failure in the host pipeline");
}

/* ------------------------------------------------------------------------ */
/* LDPC batches (ldpc.hip)                                                  */
/* ------------------------------------------------------------------------ */

EXPORT bool poporon_amd_ldpc_graph(const poporon_t *h, uint32_t *num_checks, uint32_t *num_bits, uint32_t *num_edges,
                                   const uint32_t **row_ptr, const uint32_t **col_idx,
                                   const uint32_t **inner_forward, const uint32_t **outer_forward)
{
    if (!h || h->fec_type != PPLN_FEC_LDPC)
        return fail("poporon_amd_ldpc_graph needs an LDPC handle");
    const LdpcGraph &lg = *h->ldpc;
    if (num_checks)
        *num_checks = lg.num_checks;
    if (num_bits)
        *num_bits = lg.num_bits;
    if (num_edges)
        *num_edges = lg.num_edges;
    if (row_ptr)
        *row_ptr = lg.row_ptr.data();
    if (col_idx)
        *col_idx = lg.col_idx.data();
    if (inner_forward)
        *inner_forward = lg.inner ? lg.inner_forward.data() : nullptr;
    if (outer_forward)
        *outer_forward = lg.outer ? lg.outer_forward.data() : nullptr;
    return true;
}

/* every LDPC batch entry point: an LDPC handle whose code is served, rows
 * that do not overlap, the device context */
static bool ldpc_enter(poporon_t *h, const char *what, size_t data_stride, size_t parity_stride, size_t count,
                       bool reads_parity = true)
{
    if (!h)
        return fail("NULL handle");
    if (h->fec_type != PPLN_FEC_LDPC)
        return fail("%s serves LDPC handles", what);
    if (count > 1 && (data_stride < h->ldpc->info_bytes || (reads_parity && parity_stride < h->ldpc->parity_bytes)))
        return fail("%s: data_stride / parity_stride below the row sizes (%u / %u bytes)", what,
                    (unsigned)h->ldpc->info_bytes, (unsigned)h->ldpc->parity_bytes);
    return batch_enter(h);
}

static bool ldpc_launch_decode(poporon_t *h, uint8_t *d_data, size_t ds, const uint8_t *d_par, size_t ps,
                               const int8_t *d_llr, size_t ls, size_t count, uint8_t *d_ok, uint32_t *d_it,
                               uint8_t *d_hard, size_t hs, hipStream_t s)
{
    GpuCtx &g = h->gpu;
    if (count == 0)
        return true;
    const bool lds = ldpc_use_lds(h);
    if (lds && ldpck_decode_lds_bytes(&h->ldev) > ldpck_decode_lds_room())
        return fail("POPORON_AMD_LDPC_PATH=lds: the code's messages (%zu bytes) do not fit the %zu bytes the kernel "
                    "leaves of the CU's %u bytes of LDS",
                    ldpck_decode_lds_bytes(&h->ldev), ldpck_decode_lds_room(), (unsigned)LDPC_LDS_MAX);
    const uint32_t grid = ldpck_decode_grid(&h->ldev, count, g.num_cu, lds);
    if (!lds && (!ldpc_reserve(h, count) || !rem_acquire(g, s)))
        return false;
    KernelTimer t(g, POPORON_AMD_KERNEL_LDPC_DECODE, s);
    HIP_OK(ldpck_decode(&h->ldev, d_data, ds, d_par, ps, d_llr, ls, count, d_ok, d_it, d_hard, hs,
                        h->ldpc_max_iterations, lds, g.lws, grid, s));
    t.done();
    return lds || rem_release(g, s);
}

EXPORT bool poporon_ldpc_encode_batch_device(poporon_t *h, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                             size_t parity_stride, size_t count, void *stream)
{
    if (!ldpc_enter(h, "poporon_ldpc_encode_batch_device", data_stride, parity_stride, count))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    if (count && (!d_data || !d_parity))
        return fail("NULL argument");
    DeviceGuard dg(h->gpu.device);
    KernelTimer t(h->gpu, POPORON_AMD_KERNEL_LDPC_ENCODE, (hipStream_t)stream);
    HIP_OK(ldpck_encode(&h->ldev, d_data, data_stride, d_parity, parity_stride, count, h->gpu.num_cu,
                        (hipStream_t)stream));
    t.done();
    return true;
}

EXPORT bool poporon_ldpc_check_batch_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                            const uint8_t *d_parity, size_t parity_stride, size_t count,
                                            uint8_t *d_dirty, void *stream)
{
    if (!ldpc_enter(h, "poporon_ldpc_check_batch_device", data_stride, parity_stride, count))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    if (count && (!d_data || !d_parity || !d_dirty))
        return fail("NULL argument");
    DeviceGuard dg(h->gpu.device);
    KernelTimer t(h->gpu, POPORON_AMD_KERNEL_LDPC_CHECK, (hipStream_t)stream);
    HIP_OK(ldpck_check(&h->ldev, d_data, data_stride, d_parity, parity_stride, count, d_dirty, h->gpu.num_cu,
                       (hipStream_t)stream));
    t.done();
    return true;
}

EXPORT bool poporon_ldpc_decode_batch_device(poporon_t *h, uint8_t *d_data, size_t data_stride,
                                             const uint8_t *d_parity, size_t parity_stride, const int8_t *d_llr,
                                             size_t llr_stride, size_t count, uint8_t *d_ok, uint32_t *d_iterations,
                                             uint8_t *d_hard, size_t hard_stride, void *stream)
{
    if (!ldpc_enter(h, "poporon_ldpc_decode_batch_device", data_stride, parity_stride, count, !d_llr))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, false};
    if (count && (!d_data || !d_ok || (!d_llr && !d_parity)))
        return fail("NULL argument");
    if (count > 1 && ((d_llr && llr_stride < h->ldpc->codeword_bits) ||
                      (d_hard && hard_stride < h->ldpc->codeword_bytes)))
        return fail("llr_stride / hard_stride below the row sizes (%u / %u)", (unsigned)h->ldpc->codeword_bits,
                    (unsigned)h->ldpc->codeword_bytes);
    DeviceGuard dg(h->gpu.device);
    return ldpc_launch_decode(h, d_data, data_stride, d_parity, parity_stride, d_llr, llr_stride, count, d_ok,
                              d_iterations, d_hard, hard_stride, (hipStream_t)stream);
}

/* Host forms: chunks of rows through one pinned slot, synchronously (copy in,
 * kernel, copy out).  `in` packs chunk [c0, c0 + n) into the slot's host
 * buffer, `run` copies, launches and copies back on the slot's stream, `out`
 * hands the results to the caller's arrays. */
static const size_t kLdpcChunkBytes = (size_t)8 << 20;

template <typename In, typename Run, typename Out>
static bool ldpc_host_chunks(poporon_t *h, size_t count, size_t row_bytes, In in, Run run, Out out)
{
    const size_t chunk = std::max<size_t>(1, std::min(count, kLdpcChunkBytes / row_bytes));
    return host_chunks(h, &h->gpu.pipe[0], 1, count, chunk, chunk * row_bytes + 64, in, run, out,
                       "HIP failure in an LDPC host batch");
}

EXPORT bool poporon_ldpc_encode_batch(poporon_t *h, uint8_t *data, size_t data_stride, uint8_t *parity,
                                      size_t parity_stride, size_t count)
{
    if (!ldpc_enter(h, "poporon_ldpc_encode_batch", data_stride, parity_stride, count))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    if (count && (!data || !parity))
        return fail("NULL argument");
    DeviceGuard dg(h->gpu.device);
    const size_t ib = h->ldpc->info_bytes, pb = h->ldpc->parity_bytes, w = ib + pb;
    const bool rewrites = h->ldpc->inner || h->ldpc->outer;
    return ldpc_host_chunks(
        h, count, w,
        [&](uint8_t *hb, size_t c0, size_t n) { copy_rows(hb, w, data + c0 * data_stride, data_stride, ib, n); },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, n * w, hipMemcpyHostToDevice, ps.stream));
            KernelTimer t(h->gpu, POPORON_AMD_KERNEL_LDPC_ENCODE, ps.stream);
            HIP_OK(ldpck_encode(&h->ldev, ps.dev, w, ps.dev + ib, w, n, h->gpu.num_cu, ps.stream));
            t.done();
            HIP_OK(hipMemcpyAsync(ps.host, ps.dev, n * w, hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) {
            if (rewrites)
                copy_rows(data + c0 * data_stride, data_stride, hb, w, ib, n);
            copy_rows(parity + c0 * parity_stride, parity_stride, hb + ib, w, pb, n);
        });
}

EXPORT bool poporon_ldpc_check_batch(poporon_t *h, const uint8_t *data, size_t data_stride, const uint8_t *parity,
                                     size_t parity_stride, size_t count, uint8_t *dirty)
{
    if (!ldpc_enter(h, "poporon_ldpc_check_batch", data_stride, parity_stride, count))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    if (count && (!data || !parity || !dirty))
        return fail("NULL argument");
    DeviceGuard dg(h->gpu.device);
    const size_t ib = h->ldpc->info_bytes, pb = h->ldpc->parity_bytes, w = ib + pb;
    return ldpc_host_chunks(
        h, count, w + 1,
        [&](uint8_t *hb, size_t c0, size_t n) {
            copy_rows(hb, w, data + c0 * data_stride, data_stride, ib, n);
            copy_rows(hb + ib, w, parity + c0 * parity_stride, parity_stride, pb, n);
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, n * w, hipMemcpyHostToDevice, ps.stream));
            KernelTimer t(h->gpu, POPORON_AMD_KERNEL_LDPC_CHECK, ps.stream);
            HIP_OK(ldpck_check(&h->ldev, ps.dev, w, ps.dev + ib, w, n, ps.dev + n * w, h->gpu.num_cu, ps.stream));
            t.done();
            HIP_OK(hipMemcpyAsync(ps.host + n * w, ps.dev + n * w, n, hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) { memcpy(dirty + c0, hb + n * w, n); });
}

EXPORT bool poporon_ldpc_decode_batch(poporon_t *h, uint8_t *data, size_t data_stride, const uint8_t *parity,
                                      size_t parity_stride, const int8_t *llr, size_t llr_stride, size_t count,
                                      uint8_t *ok, uint32_t *iterations, uint8_t *hard, size_t hard_stride)
{
    if (!ldpc_enter(h, "poporon_ldpc_decode_batch", data_stride, parity_stride, count, !llr))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    if (count && (!data || !ok || (!llr && !parity)))
        return fail("NULL argument");
    DeviceGuard dg(h->gpu.device);
    const size_t ib = h->ldpc->info_bytes, pb = h->ldpc->parity_bytes, w = ib + pb;
    const size_t lb = llr ? h->ldpc->codeword_bits : 0, hb_ = hard ? h->ldpc->codeword_bytes : 0;
    if (count > 1 && ((llr && llr_stride < lb) || (hard && hard_stride < hb_)))
        return fail("llr_stride / hard_stride below the row sizes (%u / %u)", (unsigned)h->ldpc->codeword_bits,
                    (unsigned)h->ldpc->codeword_bytes);
    /* slot layout for n rows: [rows w n | llr lb n | hard hb n | iterations 4 n (4-aligned) | ok n] */
    auto o_hard = [&](size_t n) { return n * (w + lb); };
    auto o_it = [&](size_t n) { return (n * (w + lb + hb_) + 3) & ~(size_t)3; };
    auto o_ok = [&](size_t n) { return o_it(n) + 4 * n; };
    return ldpc_host_chunks(
        h, count, w + lb + hb_ + 5 + 4,
        [&](uint8_t *hb, size_t c0, size_t n) {
            copy_rows(hb, w, data + c0 * data_stride, data_stride, ib, n);
            if (parity)
                copy_rows(hb + ib, w, parity + c0 * parity_stride, parity_stride, pb, n);
            if (llr)
                copy_rows(hb + n * w, lb, (const uint8_t *)llr + c0 * llr_stride, llr_stride, lb, n);
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, n * (w + lb), hipMemcpyHostToDevice, ps.stream));
            if (!ldpc_launch_decode(h, ps.dev, w, ps.dev + ib, w, llr ? (const int8_t *)(ps.dev + n * w) : nullptr, lb,
                                    n, ps.dev + o_ok(n), (uint32_t *)(ps.dev + o_it(n)),
                                    hard ? ps.dev + o_hard(n) : nullptr, hb_, ps.stream))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host, ps.dev, n * w, hipMemcpyDeviceToHost, ps.stream));
            HIP_OK(hipMemcpyAsync(ps.host + o_hard(n), ps.dev + o_hard(n), o_ok(n) + n - o_hard(n),
                                  hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) {
            copy_rows(data + c0 * data_stride, data_stride, hb, w, ib, n); /* failed rows come back unchanged */
            if (hard)
                copy_rows(hard + c0 * hard_stride, hard_stride, hb + o_hard(n), hb_, hb_, n);
            if (iterations)
                memcpy(iterations + c0, hb + o_it(n), 4 * n);
            memcpy(ok + c0, hb + o_ok(n), n);
        });
}

/* ------------------------------------------------------------------------ */
/* symbol-interleaved frames: layout kernels around the row kernels         */
/* ------------------------------------------------------------------------ */

/*
 * A frame holds `depth` codewords interleaved symbol by symbol (poporon_amd.h).
 * The codec kernels are untouched: a chunk of frames is gathered into staging
 * rows (rs_interleave.hip; size + num_roots bytes back to back, the wire rows
 * the codec kernels are measured on, in RS_ILV_ROW bytes per codeword), the
 * row launchers run there on codewords c = f*depth + i, and the results are
 * scattered back -- the parity for an encode, both regions for a decode,
 * nothing for a check.  Depth 1 is the row layout and runs in place.  A chunk
 * is at most ilv_chunk codewords, in whole frames and at least one frame;
 * larger batches run chunk after chunk on the caller's stream.  The staging
 * buffer is the handle's, grown on demand, and shares the split workspace's
 * ordering across streams (rem_acquire / rem_release).
 */
static bool ensure_ilv(poporon_t *h, size_t codewords)
{
    return ensure_buf(h->gpu, h->gpu.ilv, codewords, RS_ILV_ROW, RS_ILV_MAX_DEPTH);
}

/* The report calls' snapshot buffer (rs_report.hip): the rows of a chunk as
 * they were before the decode, wire rows in RS_ILV_ROW bytes per codeword,
 * the handle's, grown on demand and ordered across streams as ilv is.  At
 * least 64 codewords, so that the 16-byte slot at the end of the rows lies
 * inside it. */
static bool ensure_rep(poporon_t *h, size_t codewords)
{
    return ensure_buf(h->gpu, h->gpu.rep, codewords, RS_ILV_ROW, RS_ILV_MAX_DEPTH);
}

/* list rows sit on a 16-byte aligned base at a stride that is a multiple of 16: the 32-erasure kernel's fast route */
static size_t plane_list_stride(const poporon_t *h) { return rs_ws_round16(h->rs->num_roots); }

/* The plane and product calls' erasure lists (rs_planes.hip, rs_product.hip): plist.cap list rows, then plist.cap
 * counts */
static bool ensure_plist(poporon_t *h, size_t codewords)
{
    return ensure_buf(h->gpu, h->gpu.plist, codewords, plane_list_stride(h) + 1, 0);
}

/* every form's first refusals: a handle, and an RS one; then the size of its rows */
static bool rs_handle(const poporon_t *h, const char *what)
{
    if (!h)
        return fail("%s: NULL handle", what);
    if (h->fec_type != PPLN_FEC_RS)
        return fail("%s serves RS handles", what);
    return true;
}

static bool form_size(const poporon_t *h, const char *what, size_t size)
{
    return check_decode_size(h, size) || fail("%s: size %zu outside [1, %u]", what, size, (unsigned)kmax(h));
}

/* after the argument checks: run(stream) inside the batch scope on the handle's device.  A device form enqueues on
 * the caller's stream and returns; a host form (host: no stream) returns when its work has run. */
template <class F> static bool form_scope(poporon_t *h, size_t count, void *stream, bool host, F &&run)
{
    if (count == 0)
        return true;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, (hipStream_t)stream, host};
    DeviceGuard dg(h->gpu.device);
    return run((hipStream_t)stream);
}

/* the reserve calls: the handle's device context, then run() on its device */
template <class F> static bool reserve_scope(poporon_t *h, const char *what, F &&run)
{
    if (!h)
        return fail("NULL handle");
    if (!rs_handle(h, what) || !gpu_init(h))
        return false;
    DeviceGuard dg(h->gpu.device);
    return run();
}

/* where a report goes: num[c], pos / val[c * stride .. + num_roots) */
struct RepOut {
    uint8_t *num, *pos, *val;
    size_t stride;
};

/* n rows -> the snapshot buffer.  Rows that are wire rows already (parity
 * behind the message, both strides size + nr) are one device copy, stamped
 * with the timer's events by hand since no kernel of ours runs; any other
 * placement is gathered by rs_snapshot_k. */
static bool rep_snapshot(poporon_t *h, const DecodeCall &c)
{
    GpuCtx &g = h->gpu;
    const uint32_t nr = h->rs->num_roots;
    const uint8_t *d = c.data, *p = c.par;
    const size_t ds = c.ds, ps = c.ps, size = c.size, n = c.count, w = size + nr;
    hipStream_t s = c.s;
    KernelTimer t(g, POPORON_AMD_KERNEL_SNAPSHOT, s);
    if (p == d + size && ds == w && ps == w) {
        if (t.a)
            HIP_OK(hipEventRecord(t.a, s));
        HIP_OK(hipMemcpyAsync(g.rep.p, d, n * w, hipMemcpyDeviceToDevice, s));
        if (t.a) {
            HIP_OK(hipEventRecord(t.b, s));
            rs_launch_timer.n = 1;
        }
    } else {
        HIP_OK(rsk_snapshot(d, ds, p, ps, g.rep.p, (uint32_t)size, nr, n, s));
    }
    t.done();
    return true;
}

/* the n rows as they are now against the snapshot buffer */
static bool rep_diff(poporon_t *h, const DecodeCall &c, const RepOut &o, size_t c0)
{
    STAGE(h->gpu, POPORON_AMD_KERNEL_REPORT, c.s,
          rsk_report(c.data, c.ds, c.par, c.ps, h->gpu.rep.p, (uint32_t)c.size, h->rs->num_roots, c.count, o.num + c0,
                     o.pos + c0 * o.stride, o.val + c0 * o.stride, o.stride, c.s));
    return true;
}

/*
 * The staged-chunk driver: what the interleaved, report, convolutional-check
 * and plane calls have in common.  A call is an operation on `count` codewords,
 * `chunk` at a time, and a layout of two callables in the manner of
 * host_chunks: gather(c0, n, rows) says where the rows of codewords
 * [c0, c0 + n) are, after bringing them there, and scatter(c0, n) takes them
 * back (not called after a check).  Everything between is here and only here:
 * the snapshot buffer of a report, the one DecodeCall of a chunk with every
 * per-codeword array advanced by c0, snapshot / decode / diff, encode or check,
 * and the ordering across streams of the handle's shared buffers -- a call whose
 * rows are staged (ilv, with it plist) or that reports (rep) waits for rem_done
 * before its first writer and records it behind its last reader; a call on the
 * caller's own rows without a report does neither.
 */
enum FormOp { FORM_ENCODE, FORM_DECODE, FORM_CHECK };

struct FormCall {
    FormOp op;
    size_t size, count, chunk; /* count, chunk: codewords */
    bool staged;               /* the rows are the handle's staging rows (ilv), which the driver sizes */
    const uint8_t *pos;        /* FORM_DECODE: erasure lists, per codeword or (shared_lists) one for all */
    size_t pos_stride;
    const uint8_t *cnt;
    bool shared_lists;
    uint8_t *ok, *cor;
    uint8_t *dirty; /* FORM_CHECK: its flags; FORM_DECODE: non-NULL for a check of the decoded rows */
    RepOut rep;     /* FORM_DECODE: the report arrays (num NULL: none) */
};

struct FormRows {
    uint8_t *data;
    size_t ds;
    uint8_t *par;
    size_t ps;
};

template <class Gather, class Scatter>
static bool form_chunks(poporon_t *h, const FormCall &c, hipStream_t s, Gather &&gather, Scatter &&scatter)
{
    GpuCtx &g = h->gpu;
    const bool report = c.op == FORM_DECODE && c.rep.num, shared = c.staged || report;
    const size_t n0 = std::min(c.count, c.chunk);
    if ((report && !ensure_rep(h, n0)) || (c.staged && !ensure_ilv(h, n0)) || (shared && !rem_acquire(g, s)))
        return false;
    for (size_t c0 = 0; c0 < c.count; c0 += c.chunk) {
        const size_t n = std::min(c.chunk, c.count - c0), l0 = c.shared_lists ? 0 : c0;
        FormRows r;
        if (!gather(c0, n, r))
            return false;
        if (c.op == FORM_ENCODE) {
            if (!launch_encode(h, r.data, r.ds, r.par, r.ps, c.size, n, s))
                return false;
        } else if (c.op == FORM_DECODE) {
            const DecodeCall d = {.data = r.data, .ds = r.ds, .par = r.par, .ps = r.ps, .size = c.size, .count = n,
                                  .pos8 = c.pos ? c.pos + l0 * c.pos_stride : nullptr, .pos_stride = c.pos_stride,
                                  .cnt = c.pos ? c.cnt + l0 : nullptr, .ok = c.ok + c0,
                                  .corrected = c.cor ? c.cor + c0 : nullptr, .s = s};
            /* report: the rows as gathered are the snapshot */
            if ((report && !rep_snapshot(h, d)) || !launch_decode(h, d) || (report && !rep_diff(h, d, c.rep, c0)))
                return false;
        }
        if (c.op != FORM_ENCODE && c.dirty && !launch_check(h, r.data, r.ds, r.par, r.ps, c.size, n, c.dirty + c0, s))
            return false;
        if (c.op != FORM_CHECK && !scatter(c0, n))
            return false;
    }
    return !shared || rem_release(g, s);
}

struct IlvCall {
    FormOp op;
    uint8_t *data;
    size_t ds;
    uint8_t *par;
    size_t ps;
    size_t size, depth, count; /* count: frames */
    const uint8_t *pos;
    size_t pos_stride;
    const uint8_t *cnt;
    uint8_t *ok, *cor, *dirty;
    RepOut rep; /* FORM_DECODE: the report arrays (num NULL: none) */
};

static size_t ilv_chunk_frames(const poporon_t *h, size_t depth) { return std::max<size_t>(1, h->ilv_chunk / depth); }

/* the checks every interleaved entry point makes before it touches the GPU */
static bool ilv_args(const poporon_t *h, const char *what, const IlvCall &c)
{
    if (!rs_handle(h, what))
        return false;
    if (c.count && (!c.data || !c.par || (c.op == FORM_DECODE && !c.ok) || (c.op == FORM_CHECK && !c.dirty)))
        return fail("%s: NULL argument", what);
    if (c.depth < 1 || c.depth > RS_ILV_MAX_DEPTH)
        return fail("%s: depth %zu outside [1, %u]", what, c.depth, (unsigned)RS_ILV_MAX_DEPTH);
    if (!form_size(h, what, c.size))
        return false;
    const size_t nr = h->rs->num_roots;
    if (c.ds < c.size * c.depth)
        return fail("%s: data_stride %zu < size * depth = %zu", what, c.ds, c.size * c.depth);
    if (c.ps < nr * c.depth)
        return fail("%s: parity_stride %zu < num_roots * depth = %zu", what, c.ps, nr * c.depth);
    if (c.pos && (!c.cnt || c.pos_stride < nr))
        return fail("%s: erasure batch needs counts and positions_stride >= num_roots", what);
    return true;
}

static bool rep_run(poporon_t *h, const DecodeCall &c, const RepOut &o);

/* The wire form's device image (rs_device.h: to_code, to_wire, the sequence
 * continued round), the handle's, uploaded by the first call after a form was
 * set.  No launch reads the old image by then: poporon_amd_set_wire_form has
 * waited for them. */
static bool ensure_wire(poporon_t *h)
{
    GpuCtx &g = h->gpu;
    if (!h->wf_set || g.wire_ok)
        return true;
    const size_t xlen = h->wf_seq.size(), bytes = RS_ILV_WIRE_BYTES(xlen);
    if (g.wire_cap < bytes) {
        HIP_OK(hipFree(g.wire));
        g.wire = nullptr;
        g.wire_cap = 0;
        HIP_OK(hipMalloc((void **)&g.wire, bytes));
        g.wire_cap = bytes;
    }
    std::vector<uint8_t> img(bytes);
    memcpy(img.data(), h->wf_code, 256);
    memcpy(img.data() + 256, h->wf_wire, 256);
    for (size_t i = 0; i + 512 < bytes; i++)
        img[512 + i] = h->wf_seq[i % xlen];
    HIP_OK(hipMemcpy(g.wire, img.data(), bytes, hipMemcpyHostToDevice));
    g.wire_ok = true;
    return true;
}

/* device pointers; the caller holds the batch scope and the device */
static bool ilv_run(poporon_t *h, const IlvCall &c, hipStream_t s)
{
    GpuCtx &g = h->gpu;
    const uint32_t nr = h->rs->num_roots, size = (uint32_t)c.size, depth = (uint32_t)c.depth;
    /* with a wire form every byte changes on its way in and out: depth 1 is staged too */
    const bool mapped = h->wf_set, staged = depth > 1 || mapped, decode = c.op == FORM_DECODE;
    if (decode && c.rep.num && !staged) /* depth 1 is the row layout: the row report */
        return rep_run(h, {.data = c.data, .ds = c.ds, .par = c.par, .ps = c.ps, .size = c.size, .count = c.count,
                           .pos8 = c.pos, .pos_stride = c.pos_stride, .cnt = c.cnt, .ok = c.ok, .corrected = c.cor,
                           .s = s},
                       c.rep);
    if (mapped && !ensure_wire(h))
        return false;
    /* an encode reads the message through to_code and uses no sequence */
    const uint32_t xlen = c.op == FORM_ENCODE ? 0u : (uint32_t)h->wf_seq.size();
    /* whole frames: codewords [c0, c0 + n) are frames [c0 / depth, (c0 + n) / depth) */
    const FormCall f = {.op = c.op, .size = c.size, .count = c.count * depth,
                        .chunk = ilv_chunk_frames(h, depth) * depth, .staged = staged, .pos = c.pos,
                        .pos_stride = c.pos_stride, .cnt = c.cnt, .ok = c.ok, .cor = c.cor, .dirty = c.dirty,
                        .rep = c.rep};
    return form_chunks(
        h, f, s,
        [&](size_t c0, size_t n, FormRows &r) {
            uint8_t *fd = c.data + c0 / depth * c.ds, *fp = c.par + c0 / depth * c.ps;
            if (!staged) { /* in place: the caller's rows, and none of the handle's buffers */
                r = {fd, c.ds, fp, c.ps};
                return true;
            }
            r = {g.ilv.p, size + nr, g.ilv.p + size, size + nr}; /* wire rows */
            if (mapped)
                STAGE(g, POPORON_AMD_KERNEL_ILV_GATHER, s,
                      rsk_ilv_gather_map(fd, c.ds, fp, c.ps, g.ilv.p, size, nr, depth, n / depth, c.op != FORM_ENCODE,
                                         g.wire, xlen, s));
            else
                STAGE(g, POPORON_AMD_KERNEL_ILV_GATHER, s,
                      rsk_ilv_gather(fd, c.ds, fp, c.ps, g.ilv.p, size, nr, depth, n / depth, c.op != FORM_ENCODE, s));
            return true;
        },
        [&](size_t c0, size_t n) {
            uint8_t *fd = c.data + c0 / depth * c.ds, *fp = c.par + c0 / depth * c.ps;
            if (mapped)
                STAGE(g, POPORON_AMD_KERNEL_ILV_SCATTER, s,
                      rsk_ilv_scatter_map(g.ilv.p, fd, c.ds, fp, c.ps, size, nr, depth, n / depth, decode, g.wire, s));
            else if (staged)
                STAGE(g, POPORON_AMD_KERNEL_ILV_SCATTER, s,
                      rsk_ilv_scatter(g.ilv.p, fd, c.ds, fp, c.ps, size, nr, depth, n / depth, decode, s));
            return true;
        });
}

static bool ilv_device(poporon_t *h, const char *what, const IlvCall &c, void *stream)
{
    return ilv_args(h, what, c) &&
           form_scope(h, c.count, stream, false, [&](hipStream_t s) { return ilv_run(h, c, s); });
}

EXPORT bool poporon_encode_interleaved_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                              uint8_t *d_parity, size_t parity_stride, size_t size, size_t depth,
                                              size_t count, void *stream)
{
    const IlvCall c = {FORM_ENCODE, const_cast<uint8_t *>(d_data), data_stride, d_parity, parity_stride, size, depth,
                       count,      nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    return ilv_device(h, "poporon_encode_interleaved_device", c, stream);
}

EXPORT bool poporon_decode_interleaved_device(poporon_t *h, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                              size_t parity_stride, size_t size, size_t depth, size_t count,
                                              const uint8_t *d_positions, size_t positions_stride,
                                              const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected,
                                              void *stream)
{
    const IlvCall c = {FORM_DECODE, d_data,      data_stride,      d_parity, parity_stride, size,        depth,
                       count,      d_positions, positions_stride, d_counts, d_ok,          d_corrected, nullptr};
    return ilv_device(h, "poporon_decode_interleaved_device", c, stream);
}

EXPORT bool poporon_check_interleaved_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                             const uint8_t *d_parity, size_t parity_stride, size_t size, size_t depth,
                                             size_t count, uint8_t *d_dirty, void *stream)
{
    const IlvCall c = {FORM_CHECK, const_cast<uint8_t *>(d_data), data_stride, const_cast<uint8_t *>(d_parity),
                       parity_stride, size, depth, count, nullptr, 0, nullptr, nullptr, nullptr, d_dirty};
    return ilv_device(h, "poporon_check_interleaved_device", c, stream);
}

EXPORT bool poporon_amd_reserve_interleaved(poporon_t *h, size_t max_codewords)
{
    return reserve_scope(h, "poporon_amd_reserve_interleaved", [&] {
        /* a chunk is ilv_chunk codewords at most, or one frame where that is more */
        const size_t n = std::min(max_codewords, std::max(h->ilv_chunk, (size_t)RS_ILV_MAX_DEPTH));
        return ensure_ilv(h, n) && ensure_rem(h, n) && ensure_wire(h);
    });
}

/* Host forms: chunks of frames through one pinned slot and the device form,
 * synchronously.  Slot layout for n frames of ncw codewords, as wire blocks:
 * [frames (size + nr) depth n | to 16 | positions nr ncw | counts ncw | ok ncw | corrected ncw] */
static const size_t kIlvHostBytes = (size_t)8 << 20;

static bool ilv_host_run(poporon_t *h, const IlvCall &c)
{
    const size_t nr = h->rs->num_roots, db = c.size * c.depth, pb = nr * c.depth, fb = db + pb;
    const size_t eb = c.pos ? nr : 0; /* erasure slots per codeword */
    const size_t chunk = std::max<size_t>(1, std::min(c.count, kIlvHostBytes / (fb + c.depth * (eb + 3))));
    auto o_pos = [&](size_t n) { return rs_ws_round16(n * fb); };
    auto o_cnt = [&](size_t n) { return o_pos(n) + n * c.depth * eb; };
    auto o_ok = [&](size_t n) { return o_cnt(n) + n * c.depth; };
    auto o_cor = [&](size_t n) { return o_ok(n) + n * c.depth; };
    return host_chunks(
        h, &h->gpu.pipe[0], 1, c.count, chunk, o_cor(chunk) + chunk * c.depth,
        [&](uint8_t *hb, size_t f0, size_t n) {
            const size_t ncw = n * c.depth, c0 = f0 * c.depth;
            copy_rows(hb, fb, c.data + f0 * c.ds, c.ds, db, n);
            if (c.op != FORM_ENCODE)
                copy_rows(hb + db, fb, c.par + f0 * c.ps, c.ps, pb, n);
            if (c.pos) {
                copy_rows(hb + o_pos(n), nr, c.pos + c0 * c.pos_stride, c.pos_stride, nr, ncw);
                memcpy(hb + o_cnt(n), c.cnt + c0, ncw);
            }
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            const IlvCall d = {.op = c.op, .data = ps.dev, .ds = fb, .par = ps.dev + db, .ps = fb, .size = c.size,
                               .depth = c.depth, .count = n, .pos = c.pos ? ps.dev + o_pos(n) : nullptr,
                               .pos_stride = nr, .cnt = ps.dev + o_cnt(n), .ok = ps.dev + o_ok(n),
                               .cor = ps.dev + o_cor(n)};
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, o_ok(n), hipMemcpyHostToDevice, ps.stream));
            if (!ilv_run(h, d, ps.stream))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host, ps.dev, n * fb, hipMemcpyDeviceToHost, ps.stream));
            if (c.op == FORM_DECODE)
                HIP_OK(hipMemcpyAsync(ps.host + o_ok(n), ps.dev + o_ok(n), 2 * n * c.depth, hipMemcpyDeviceToHost,
                                      ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t f0, size_t n) {
            const size_t ncw = n * c.depth, c0 = f0 * c.depth;
            copy_rows(c.par + f0 * c.ps, c.ps, hb + db, fb, pb, n);
            if (c.op == FORM_DECODE) {
                copy_rows(c.data + f0 * c.ds, c.ds, hb, fb, db, n);
                memcpy(c.ok + c0, hb + o_ok(n), ncw);
                if (c.cor)
                    memcpy(c.cor + c0, hb + o_cor(n), ncw);
            }
        },
        "HIP failure in an interleaved host batch");
}

static bool ilv_host(poporon_t *h, const char *what, const IlvCall &c)
{
    return ilv_args(h, what, c) &&
           form_scope(h, c.count, nullptr, true, [&](hipStream_t) { return ilv_host_run(h, c); });
}

EXPORT bool poporon_encode_interleaved(poporon_t *h, const uint8_t *data, size_t data_stride, uint8_t *parity,
                                       size_t parity_stride, size_t size, size_t depth, size_t count)
{
    const IlvCall c = {FORM_ENCODE, const_cast<uint8_t *>(data), data_stride, parity, parity_stride, size, depth,
                       count,      nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    return ilv_host(h, "poporon_encode_interleaved", c);
}

EXPORT bool poporon_decode_interleaved(poporon_t *h, uint8_t *data, size_t data_stride, uint8_t *parity,
                                       size_t parity_stride, size_t size, size_t depth, size_t count,
                                       const uint8_t *positions, size_t positions_stride, const uint8_t *counts,
                                       uint8_t *ok, uint8_t *corrected)
{
    const IlvCall c = {FORM_DECODE, data,      data_stride,      parity, parity_stride, size,      depth,
                       count,      positions, positions_stride, counts, ok,            corrected, nullptr};
    return ilv_host(h, "poporon_decode_interleaved", c);
}

/* ------------------------------------------------------------------------ */
/* wire form of the interleaved calls: symbol map and receive-side sequence  */
/* ------------------------------------------------------------------------ */

static bool wire_handle(const poporon_t *h, const char *what)
{
    if (!rs_handle(h, what))
        return false;
    if (h->rs->gf->symbol_size != 8)
        return fail("%s: a wire form maps bytes; the handle's symbol_size is %u, not 8", what,
                    (unsigned)h->rs->gf->symbol_size);
    return true;
}

EXPORT bool poporon_amd_set_wire_form(poporon_t *h, const uint8_t to_code[256], const uint8_t to_wire[256],
                                      const uint8_t *xor_seq, size_t xor_len)
{
    const char *what = "poporon_amd_set_wire_form";
    if (!wire_handle(h, what))
        return false;
    if (!to_code != !to_wire)
        return fail("%s: to_code and to_wire are both given or both NULL", what);
    if (!xor_seq != !xor_len)
        return fail("%s: xor_seq and xor_len are both given or NULL and 0", what);
    if (xor_len > RS_ILV_XOR_MAX)
        return fail("%s: xor_len %zu outside [1, %u]", what, xor_len, (unsigned)RS_ILV_XOR_MAX);
    if (to_code)
        for (unsigned v = 0; v < 256; v++)
            if (to_wire[to_code[v]] != v)
                return fail("%s: to_wire[to_code[%u]] = %u: the maps are not mutually inverse", what, v,
                            (unsigned)to_wire[to_code[v]]);
    /* launches already enqueued keep the form they were given: the device image
     * is replaced (by the next call's ensure_wire) only after they have run */
    GpuCtx &g = h->gpu;
    if (g.ready && g.wire) {
        DeviceGuard dg(g.device);
        if (g.rem_pending)
            HIP_OK(hipEventSynchronize(g.rem_done));
        g.rem_pending = false;
    }
    g.wire_ok = false;
    h->wf_map = to_code != nullptr;
    for (unsigned v = 0; v < 256; v++) {
        h->wf_code[v] = to_code ? to_code[v] : (uint8_t)v;
        h->wf_wire[v] = to_wire ? to_wire[v] : (uint8_t)v;
    }
    h->wf_seq.assign(xor_seq, xor_seq + xor_len);
    h->wf_set = h->wf_map || xor_len;
    return true;
}

/* GF(2^8) by 0x187 with alpha = 2: CCSDS 131.0-B's field, whatever the handle's */
static uint8_t ccsds_mul(uint8_t a, uint8_t b)
{
    unsigned r = 0, x = a;
    for (unsigned i = 0; i < 8; i++, x = (x << 1) ^ ((x & 0x80u) ? 0x187u : 0u))
        if (b >> i & 1u)
            r ^= x;
    return (uint8_t)r;
}

EXPORT bool poporon_amd_set_wire_form_ccsds(poporon_t *h, bool dual_basis, bool randomizer)
{
    if (!wire_handle(h, "poporon_amd_set_wire_form_ccsds"))
        return false;
    uint8_t code[256], wire[256], seq[255];
    if (dual_basis) {
        /* bit 7-i of to_wire[u] = Tr(u beta^i), beta = alpha^117, Tr(a) = a + a^2 + ... + a^128 */
        uint8_t beta = 1, bi[8];
        for (unsigned i = 0; i < 117; i++)
            beta = ccsds_mul(beta, 2);
        bi[0] = 1;
        for (unsigned i = 1; i < 8; i++)
            bi[i] = ccsds_mul(bi[i - 1], beta);
        for (unsigned u = 0; u < 256; u++) {
            unsigned z = 0;
            for (unsigned i = 0; i < 8; i++) {
                uint8_t p = ccsds_mul((uint8_t)u, bi[i]), tr = 0;
                for (unsigned k = 0; k < 8; k++, p = ccsds_mul(p, p))
                    tr ^= p;
                z |= (unsigned)(tr & 1u) << (7 - i);
            }
            wire[u] = (uint8_t)z;
        }
        for (unsigned u = 0; u < 256; u++)
            code[wire[u]] = (uint8_t)u;
    }
    if (randomizer) {
        /* h(x) = x^8 + x^7 + x^5 + x^3 + 1 from the all-ones state: out s0, in s0^s3^s5^s7; MSB first */
        unsigned s = 0xFFu; /* bit k: s_k */
        for (unsigned n = 0; n < 255; n++) {
            unsigned b = 0;
            for (unsigned k = 0; k < 8; k++) {
                b = b << 1 | (s & 1u);
                const unsigned in = (s ^ s >> 3 ^ s >> 5 ^ s >> 7) & 1u;
                s = s >> 1 | in << 7;
            }
            seq[n] = (uint8_t)b;
        }
    }
    return poporon_amd_set_wire_form(h, dual_basis ? code : nullptr, dual_basis ? wire : nullptr,
                                     randomizer ? seq : nullptr, randomizer ? 255 : 0);
}

EXPORT bool poporon_amd_get_wire_form(const poporon_t *h, uint8_t to_code[256], uint8_t to_wire[256],
                                      uint8_t *xor_seq, size_t xor_cap, size_t *xor_len)
{
    const char *what = "poporon_amd_get_wire_form";
    if (!wire_handle(h, what))
        return false;
    if (!h->wf_set)
        return fail("%s: no wire form is set", what);
    if (xor_len)
        *xor_len = h->wf_seq.size();
    if (xor_seq && xor_cap < h->wf_seq.size())
        return fail("%s: the sequence has %zu bytes, xor_cap is %zu", what, h->wf_seq.size(), xor_cap);
    if (to_code)
        memcpy(to_code, h->wf_code, 256);
    if (to_wire)
        memcpy(to_wire, h->wf_wire, 256);
    if (xor_seq && !h->wf_seq.empty())
        memcpy(xor_seq, h->wf_seq.data(), h->wf_seq.size());
    return true;
}

/* ------------------------------------------------------------------------ */
/* decode reports and erasure lists from flag planes (rs_report.hip)        */
/* ------------------------------------------------------------------------ */

/*
 * A report is "the bytes this call changed" (poporon_amd.h): per chunk of at
 * most rep_chunk codewords the rows are copied to the snapshot buffer, the
 * decode runs in place through launch_decode exactly as the plain call's does
 * (routed by the chunk's count), and rs_report_k lists where the rows now
 * differ from the snapshot.  No codec kernel knows about it, so it is the same
 * for every decode route.  Device pointers; the caller holds the batch scope
 * and the device.
 */
static bool rep_run(poporon_t *h, const DecodeCall &c, const RepOut &o)
{
    const FormCall f = {.op = FORM_DECODE, .size = c.size, .count = c.count, .chunk = h->rep_chunk, .pos = c.pos8,
                        .pos_stride = c.pos_stride, .cnt = c.cnt, .ok = c.ok, .cor = c.corrected, .rep = o};
    return form_chunks(
        h, f, c.s,
        [&](size_t c0, size_t, FormRows &r) { /* the degenerate layout: the rows are where they are */
            r = {c.data + c0 * c.ds, c.ds, c.par + c0 * c.ps, c.ps};
            return true;
        },
        [](size_t, size_t) { return true; });
}

/* what every report entry point checks about the report arrays */
static bool rep_args(const poporon_t *h, const char *what, size_t count, const RepOut &o)
{
    if (count && (!o.num || !o.pos || !o.val))
        return fail("%s: NULL report array", what);
    if (o.stride < h->rs->num_roots)
        return fail("%s: report_stride %zu < num_roots (%u)", what, o.stride, (unsigned)h->rs->num_roots);
    return true;
}

EXPORT bool poporon_decode_batch_report_device(poporon_t *h, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                               size_t parity_stride, size_t size, size_t count,
                                               const uint8_t *d_positions, size_t positions_stride,
                                               const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected,
                                               uint8_t *d_err_num, uint8_t *d_err_pos, uint8_t *d_err_val,
                                               size_t report_stride, void *stream)
{
    const char *what = "poporon_decode_batch_report_device";
    const RepOut o = {d_err_num, d_err_pos, d_err_val, report_stride};
    if (!decode_row_args(h, what, true, d_data, d_parity, size, count, d_positions, positions_stride, d_counts, d_ok) ||
        !rep_args(h, what, count, o))
        return false;
    return form_scope(h, count, stream, false, [&](hipStream_t s) {
        return rep_run(h, {.data = d_data, .ds = data_stride, .par = d_parity, .ps = parity_stride, .size = size,
                           .count = count, .pos8 = d_positions, .pos_stride = positions_stride, .cnt = d_counts,
                           .ok = d_ok, .corrected = d_corrected, .s = s},
                       o);
    });
}

EXPORT bool poporon_decode_interleaved_report_device(poporon_t *h, uint8_t *d_data, size_t data_stride,
                                                     uint8_t *d_parity, size_t parity_stride, size_t size,
                                                     size_t depth, size_t count, const uint8_t *d_positions,
                                                     size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                                     uint8_t *d_corrected, uint8_t *d_err_num, uint8_t *d_err_pos,
                                                     uint8_t *d_err_val, size_t report_stride, void *stream)
{
    const char *what = "poporon_decode_interleaved_report_device";
    const IlvCall c = {FORM_DECODE,  d_data,           data_stride, d_parity, parity_stride, size,
                       depth,       count,            d_positions, positions_stride,        d_counts,
                       d_ok,        d_corrected,      nullptr,     {d_err_num, d_err_pos, d_err_val, report_stride}};
    if (!ilv_args(h, what, c) || !rep_args(h, what, count, c.rep))
        return false;
    return ilv_device(h, what, c, stream);
}

EXPORT bool poporon_amd_reserve_report(poporon_t *h, size_t max_codewords)
{
    return reserve_scope(h, "poporon_amd_reserve_report", [&] {
        const size_t n = std::min(max_codewords, h->rep_chunk);
        return ensure_rep(h, n) && ensure_rem(h, n);
    });
}

/* ------------------------------------------------------------------------ */
/* convolutional-interleaver streams: layout kernels around the row kernels */
/* ------------------------------------------------------------------------ */

/*
 * A Forney interleaver of `branches` FIFOs, branch b of b*cell bytes, is an
 * index map (poporon_amd.h, rs_conv.hip): the calls are stateless, and each
 * touches only the bytes of its own codewords inside its span.  The codec
 * kernels are untouched.  A decode gathers the stream straight into the
 * caller's rows and decodes there; an encode writes the caller's parity rows
 * and scatters data and parity; a check gathers chunks into the staging rows
 * of the interleaved calls, each chunk its own window of the stream.
 */
struct ConvCall {
    uint8_t *stream;
    size_t branches, cell, phase;
    uint8_t *data;
    size_t ds;
    uint8_t *par;
    size_t ps;
    size_t size, count;
    bool need_rows;   /* false: the check, which has no rows */
    bool need_parity; /* the codec calls */
};

/* span = count*row_bytes + (branches-1)*cell*branches; false on arguments out of range or overflow */
static bool conv_span(size_t row_bytes, size_t count, size_t branches, size_t cell, size_t &span)
{
    if (row_bytes < 1 || branches < 1 || branches > RS_CONV_MAX_BRANCHES || cell < 1 || cell > RS_CONV_MAX_CELL)
        return false;
    const size_t holes = (branches - 1) * cell * branches;
    if (count > ((size_t)-1 - holes) / row_bytes)
        return false;
    span = count * row_bytes + holes;
    return true;
}

EXPORT size_t poporon_amd_conv_span(size_t row_bytes, size_t count, size_t branches, size_t cell)
{
    size_t span;
    return conv_span(row_bytes, count, branches, cell, span) ? span : 0;
}

EXPORT size_t poporon_amd_conv_tile(size_t row_bytes, size_t branches, size_t cell)
{
    if (row_bytes > 255 || branches > RS_CONV_MAX_BRANCHES || cell > RS_CONV_MAX_CELL)
        return 0;
    return rsk_conv_tile((uint32_t)row_bytes, (uint32_t)branches, (uint32_t)cell);
}

/* the checks every convolutional entry point makes before it touches the GPU */
static bool conv_args(const poporon_t *h, const char *what, const ConvCall &c)
{
    if (!rs_handle(h, what))
        return false;
    if (c.count && (!c.stream || (c.need_rows && !c.data) || (c.need_parity && !c.par)))
        return fail("%s: NULL argument", what);
    if (c.branches < 1 || c.branches > RS_CONV_MAX_BRANCHES)
        return fail("%s: branches %zu outside [1, %u]", what, c.branches, (unsigned)RS_CONV_MAX_BRANCHES);
    if (c.cell < 1 || c.cell > RS_CONV_MAX_CELL)
        return fail("%s: cell %zu outside [1, %u]", what, c.cell, (unsigned)RS_CONV_MAX_CELL);
    if (c.phase >= c.branches)
        return fail("%s: phase %zu >= branches %zu", what, c.phase, c.branches);
    if (!form_size(h, what, c.size))
        return false;
    const size_t nr = h->rs->num_roots;
    if (c.need_rows && c.ds < c.size)
        return fail("%s: data_stride %zu < size %zu", what, c.ds, c.size);
    if (c.need_rows && c.par && c.ps < nr)
        return fail("%s: parity_stride %zu < num_roots %zu", what, c.ps, nr);
    size_t span;
    if (!conv_span(c.size + nr, c.count, c.branches, c.cell, span))
        return fail("%s: the span of %zu codewords overflows size_t", what, c.count);
    if (h->conv_path == RS_CONV_PATH_TILE &&
        !rsk_conv_tile((uint32_t)(c.size + nr), (uint32_t)c.branches, (uint32_t)c.cell))
        return fail("%s: POPORON_AMD_CONV_PATH=tile, and the window of %zu branches of cell %zu does not fit the LDS",
                    what, c.branches, c.cell);
    return true;
}

/* one layout pass over codewords [0, count) of the call, rows as given */
static bool conv_gather(poporon_t *h, const ConvCall &c, hipStream_t s)
{
    STAGE(h->gpu, POPORON_AMD_KERNEL_CONV_GATHER, s,
          rsk_conv_gather(c.stream, (uint32_t)c.branches, (uint32_t)c.cell, (uint32_t)c.phase, c.data, c.ds, c.par,
                          c.ps, (uint32_t)c.size, h->rs->num_roots, c.count, h->conv_path, s));
    return true;
}

static bool conv_scatter(poporon_t *h, const ConvCall &c, hipStream_t s)
{
    STAGE(h->gpu, POPORON_AMD_KERNEL_CONV_SCATTER, s,
          rsk_conv_scatter(c.data, c.ds, c.par, c.ps, (uint32_t)c.size, h->rs->num_roots, c.count,
                           (uint32_t)c.branches, (uint32_t)c.cell, (uint32_t)c.phase, c.stream, h->conv_path, s));
    return true;
}

EXPORT bool poporon_amd_conv_interleave_device(poporon_t *h, const uint8_t *d_data, size_t data_stride,
                                               const uint8_t *d_parity, size_t parity_stride, size_t size,
                                               size_t count, size_t branches, size_t cell, size_t phase,
                                               uint8_t *d_stream, void *stream)
{
    const ConvCall c = {d_stream, branches, cell, phase, const_cast<uint8_t *>(d_data), data_stride,
                        const_cast<uint8_t *>(d_parity), parity_stride, size, count, true, false};
    return conv_args(h, "poporon_amd_conv_interleave_device", c) &&
           form_scope(h, c.count, stream, false, [&](hipStream_t s) { return conv_scatter(h, c, s); });
}

EXPORT bool poporon_amd_conv_deinterleave_device(poporon_t *h, const uint8_t *d_stream, size_t branches, size_t cell,
                                                 size_t phase, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                                 size_t parity_stride, size_t size, size_t count, void *stream)
{
    const ConvCall c = {const_cast<uint8_t *>(d_stream), branches, cell, phase, d_data, data_stride, d_parity,
                        parity_stride, size, count, true, false};
    return conv_args(h, "poporon_amd_conv_deinterleave_device", c) &&
           form_scope(h, c.count, stream, false, [&](hipStream_t s) { return conv_gather(h, c, s); });
}

EXPORT bool poporon_encode_conv_device(poporon_t *h, const uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                       size_t parity_stride, size_t size, size_t count, size_t branches, size_t cell,
                                       size_t phase, uint8_t *d_stream, void *stream)
{
    const ConvCall c = {d_stream, branches, cell, phase, const_cast<uint8_t *>(d_data), data_stride, d_parity,
                        parity_stride, size, count, true, true};
    return conv_args(h, "poporon_encode_conv_device", c) && form_scope(h, c.count, stream, false, [&](hipStream_t s) {
               return launch_encode(h, c.data, c.ds, c.par, c.ps, c.size, c.count, s) && conv_scatter(h, c, s);
           });
}

/* the decode and its report form: rep.num NULL for the plain call */
static bool conv_decode(poporon_t *h, const char *what, const ConvCall &c, const uint8_t *d_positions,
                        size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected,
                        const RepOut *rep, void *stream)
{
    if (!conv_args(h, what, c) ||
        !decode_row_args(h, what, true, c.data, c.par, c.size, c.count, d_positions, positions_stride, d_counts, d_ok) ||
        (rep && !rep_args(h, what, c.count, *rep)))
        return false;
    return form_scope(h, c.count, stream, false, [&](hipStream_t s) {
        const DecodeCall d = {.data = c.data, .ds = c.ds, .par = c.par, .ps = c.ps, .size = c.size, .count = c.count,
                              .pos8 = d_positions, .pos_stride = positions_stride, .cnt = d_counts, .ok = d_ok,
                              .corrected = d_corrected, .s = s};
        return conv_gather(h, c, s) && (rep ? rep_run(h, d, *rep) : launch_decode(h, d));
    });
}

EXPORT bool poporon_decode_conv_device(poporon_t *h, const uint8_t *d_stream, size_t branches, size_t cell,
                                       size_t phase, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                       size_t parity_stride, size_t size, size_t count, const uint8_t *d_positions,
                                       size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                       uint8_t *d_corrected, void *stream)
{
    const ConvCall c = {const_cast<uint8_t *>(d_stream), branches, cell, phase, d_data, data_stride, d_parity,
                        parity_stride, size, count, true, true};
    return conv_decode(h, "poporon_decode_conv_device", c, d_positions, positions_stride, d_counts, d_ok, d_corrected,
                       nullptr, stream);
}

EXPORT bool poporon_decode_conv_report_device(poporon_t *h, const uint8_t *d_stream, size_t branches, size_t cell,
                                              size_t phase, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                              size_t parity_stride, size_t size, size_t count,
                                              const uint8_t *d_positions, size_t positions_stride,
                                              const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected,
                                              uint8_t *d_err_num, uint8_t *d_err_pos, uint8_t *d_err_val,
                                              size_t report_stride, void *stream)
{
    const ConvCall c = {const_cast<uint8_t *>(d_stream), branches, cell, phase, d_data, data_stride, d_parity,
                        parity_stride, size, count, true, true};
    const RepOut rep = {d_err_num, d_err_pos, d_err_val, report_stride};
    return conv_decode(h, "poporon_decode_conv_report_device", c, d_positions, positions_stride, d_counts, d_ok,
                       d_corrected, &rep, stream);
}

EXPORT bool poporon_check_conv_device(poporon_t *h, const uint8_t *d_stream, size_t branches, size_t cell,
                                      size_t phase, size_t size, size_t count, uint8_t *d_dirty, void *stream)
{
    const char *what = "poporon_check_conv_device";
    const ConvCall c = {const_cast<uint8_t *>(d_stream), branches, cell, phase, nullptr, 0, nullptr, 0, size, count,
                        false, false};
    if (!conv_args(h, what, c))
        return false;
    if (count && !d_dirty)
        return fail("%s: NULL argument", what);
    return form_scope(h, c.count, stream, false, [&](hipStream_t s) {
        const size_t w = size + h->rs->num_roots;
        const FormCall f = {.op = FORM_CHECK, .size = size, .count = count, .chunk = h->ilv_chunk, .staged = true,
                            .dirty = d_dirty};
        return form_chunks(
            h, f, s,
            [&](size_t c0, size_t n, FormRows &r) {
                /* chunk k is its own window of the stream: base + c0*W, phase (phase + c0*W) mod branches */
                r = {h->gpu.ilv.p, w, h->gpu.ilv.p + size, w};
                const ConvCall k = {c.stream + c0 * w, branches, cell, (phase + c0 * w % branches) % branches,
                                    r.data, w, r.par, w, size, n, true, true};
                return conv_gather(h, k, s);
            },
            [](size_t, size_t) { return true; });
    });
}

/* ------------------------------------------------------------------------ */
/* plane layout (storage stripes): layout kernels around the row kernels    */
/* ------------------------------------------------------------------------ */

/*
 * A stripe is W = size + num_roots planes, codeword c's symbol j at
 * planes[j][c] (poporon_amd.h).  plane_run is a layout of the staged-chunk
 * driver (form_chunks): per chunk of at most ilv_chunk codewords the planes are
 * gathered into the staging rows of the interleaved calls (rs_planes.hip), the
 * row launchers run there, routed by the chunk's count, and the rows are
 * scattered back -- the parity planes after an encode, every non-NULL plane
 * after a decode, nothing after a check.  The table and the lost set go to the
 * kernels by value.  A rebuild gives every codeword the same erasure list; the
 * row decoders take per-codeword lists, so the handle owns a list buffer for one
 * chunk, filled once per call.
 */
struct PlaneCall {
    FormOp op;
    uint8_t *const *planes; /* host array of size + num_roots device pointers */
    size_t size, count;
    const uint8_t *lost; /* host array */
    size_t lost_count;
    uint8_t *ok, *cor, *dirty;
    RepOut rep; /* FORM_DECODE: the report arrays (num NULL: none) */
};

/* the checks every plane entry point makes before it touches the GPU */
static bool plane_args(const poporon_t *h, const char *what, const PlaneCall &c)
{
    if (!rs_handle(h, what) || !form_size(h, what, c.size))
        return false;
    const size_t nr = h->rs->num_roots, w = c.size + nr;
    if (c.lost_count > nr)
        return fail("%s: lost_count %zu > num_roots (%zu)", what, c.lost_count, nr);
    if (c.lost_count && !c.lost)
        return fail("%s: NULL argument (the lost list)", what);
    for (size_t k = 0; k < c.lost_count; k++) {
        if (c.lost[k] >= w)
            return fail("%s: lost plane index %u >= size + num_roots = %zu", what, (unsigned)c.lost[k], w);
        if (k && c.lost[k] <= c.lost[k - 1])
            return fail("%s: the lost list is not strictly ascending at entry %zu", what, k);
    }
    if (c.count == 0)
        return true;
    if (!c.planes || (c.op == FORM_DECODE && !c.ok) || (c.op == FORM_CHECK && !c.dirty))
        return fail("%s: NULL argument", what);
    size_t k = 0, delivered = 0;
    for (size_t j = 0; j < w; j++) {
        const bool is_lost = k < c.lost_count && c.lost[k] == j;
        k += is_lost;
        if (c.op == FORM_ENCODE && j >= c.size)
            delivered += c.planes[j] != nullptr;
        else if (!c.planes[j] && !is_lost)
            return fail("%s: NULL plane %zu", what, j);
    }
    if (c.op == FORM_ENCODE && !delivered)
        return fail("%s: every parity plane is NULL", what);
    return true;
}

/* device pointers in the table; the caller holds the batch scope and the device */
static bool plane_run(poporon_t *h, const PlaneCall &c, hipStream_t s)
{
    GpuCtx &g = h->gpu;
    const uint32_t nr = h->rs->num_roots, size = (uint32_t)c.size, w = size + nr;
    const size_t chunk = h->ilv_chunk, n0 = std::min(c.count, chunk), ls = plane_list_stride(h);
    uint32_t lost[8] = {};
    for (size_t k = 0; k < c.lost_count; k++)
        lost[c.lost[k] >> 5] |= 1u << (c.lost[k] & 31u);
    /* the planes a pass touches: the message on the way into an encode, all of them otherwise; on the way out
     * the parity of an encode, all of a decode */
    const uint32_t gfirst = 0, glast = c.op == FORM_ENCODE ? size : w;
    const uint32_t sfirst = c.op == FORM_ENCODE ? size : 0, slast = w;
    uintptr_t low = 0; /* every entry a multiple of 16: the kernels whose plane runs are whole slots */
    for (uint32_t j = 0; j < w; j++)
        low |= reinterpret_cast<uintptr_t>(c.planes[j]);
    if (c.lost_count && !ensure_plist(h, n0))
        return false;
    /* one list, filled inside the first chunk's gather, serves every chunk; a decode with d_dirty checks its rows */
    const FormCall f = {.op = c.op, .size = size, .count = c.count, .chunk = h->ilv_chunk, .staged = true,
                        .pos = c.lost_count ? g.plist.p : nullptr, .pos_stride = ls,
                        .cnt = c.lost_count ? g.plist.p + g.plist.cap * ls : nullptr, .shared_lists = true, .ok = c.ok,
                        .cor = c.cor, .dirty = c.dirty, .rep = c.rep};
    return form_chunks(
        h, f, s,
        [&](size_t c0, size_t n, FormRows &r) {
            r = {g.ilv.p, w, g.ilv.p + size, w};
            KernelTimer t(g, POPORON_AMD_KERNEL_PLANE_GATHER, s);
            if (c0 == 0 && c.lost_count)
                HIP_OK(rsk_plane_lists(lost, (uint32_t)c.lost_count, g.plist.p, (uint32_t)ls,
                                       g.plist.p + g.plist.cap * ls, n0, s));
            HIP_OK(rsk_plane_gather(c.planes, lost, w, gfirst, glast, c0, r.data, n, ((low | c0) & 15u) == 0, s));
            t.done();
            return true;
        },
        [&](size_t c0, size_t n) {
            STAGE(g, POPORON_AMD_KERNEL_PLANE_SCATTER, s,
                  rsk_plane_scatter(g.ilv.p, c.planes, w, sfirst, slast, c0, n, ((low | c0) & 15u) == 0, s));
            return true;
        });
}

static bool plane_device(poporon_t *h, const char *what, const PlaneCall &c, void *stream)
{
    if (!plane_args(h, what, c) || (c.rep.num && !rep_args(h, what, c.count, c.rep)))
        return false;
    return form_scope(h, c.count, stream, false, [&](hipStream_t s) { return plane_run(h, c, s); });
}

EXPORT size_t poporon_amd_plane_tile(size_t row_bytes)
{
    return row_bytes > 255 ? 0 : rsk_plane_tile((uint32_t)row_bytes);
}

EXPORT bool poporon_amd_reserve_planes(poporon_t *h, size_t max_codewords)
{
    return reserve_scope(h, "poporon_amd_reserve_planes", [&] {
        const size_t n = std::min(max_codewords, h->ilv_chunk);
        return ensure_plist(h, n) && ensure_ilv(h, n) && ensure_rem(h, n);
    });
}

EXPORT bool poporon_encode_planes_device(poporon_t *h, uint8_t *const *planes, size_t size, size_t count, void *stream)
{
    const PlaneCall c = {FORM_ENCODE, planes, size, count, nullptr, 0, nullptr, nullptr, nullptr, {}};
    return plane_device(h, "poporon_encode_planes_device", c, stream);
}

EXPORT bool poporon_decode_planes_device(poporon_t *h, uint8_t *const *planes, size_t size, size_t count,
                                         const uint8_t *lost, size_t lost_count, uint8_t *d_ok, uint8_t *d_corrected,
                                         uint8_t *d_dirty, void *stream)
{
    const PlaneCall c = {FORM_DECODE, planes, size, count, lost, lost_count, d_ok, d_corrected, d_dirty, {}};
    return plane_device(h, "poporon_decode_planes_device", c, stream);
}

EXPORT bool poporon_decode_planes_report_device(poporon_t *h, uint8_t *const *planes, size_t size, size_t count,
                                                const uint8_t *lost, size_t lost_count, uint8_t *d_ok,
                                                uint8_t *d_corrected, uint8_t *d_dirty, uint8_t *d_err_num,
                                                uint8_t *d_err_pos, uint8_t *d_err_val, size_t report_stride,
                                                void *stream)
{
    const char *what = "poporon_decode_planes_report_device";
    const PlaneCall c = {FORM_DECODE, planes, size, count, lost, lost_count, d_ok, d_corrected, d_dirty,
                         {d_err_num, d_err_pos, d_err_val, report_stride}};
    /* the plain call is the one without report arrays: here they are required */
    if (h && h->fec_type == PPLN_FEC_RS && !rep_args(h, what, count, c.rep))
        return false;
    return plane_device(h, what, c, stream);
}

EXPORT bool poporon_check_planes_device(poporon_t *h, const uint8_t *const *planes, size_t size, size_t count,
                                        uint8_t *d_dirty, void *stream)
{
    const PlaneCall c = {FORM_CHECK, const_cast<uint8_t *const *>(planes), size, count, nullptr, 0, nullptr, nullptr,
                         d_dirty, {}};
    return plane_device(h, "poporon_check_planes_device", c, stream);
}

/* The strided forms: one buffer, message plane j at d_data + j*data_plane_stride, parity plane p at d_parity +
 * p*parity_plane_stride.  They fill a table on the host and take the table forms' path. */
static bool plane_strided(poporon_t *h, const char *what, PlaneCall c, const uint8_t *d_data, size_t ds,
                          const uint8_t *d_parity, size_t ps, void *stream)
{
    if (!rs_handle(h, what) || !form_size(h, what, c.size))
        return false;
    if (c.count && (!d_data || !d_parity))
        return fail("%s: NULL argument", what);
    const size_t nr = h->rs->num_roots;
    std::vector<uint8_t *> tab(c.size + nr);
    for (size_t j = 0; j < c.size; j++)
        tab[j] = const_cast<uint8_t *>(d_data) + j * ds;
    for (size_t p = 0; p < nr; p++)
        tab[c.size + p] = const_cast<uint8_t *>(d_parity) + p * ps;
    c.planes = tab.data();
    return plane_device(h, what, c, stream);
}

EXPORT bool poporon_encode_planes_strided_device(poporon_t *h, const uint8_t *d_data, size_t data_plane_stride,
                                                 uint8_t *d_parity, size_t parity_plane_stride, size_t size,
                                                 size_t count, void *stream)
{
    const PlaneCall c = {FORM_ENCODE, nullptr, size, count, nullptr, 0, nullptr, nullptr, nullptr, {}};
    return plane_strided(h, "poporon_encode_planes_strided_device", c, d_data, data_plane_stride, d_parity,
                         parity_plane_stride, stream);
}

EXPORT bool poporon_decode_planes_strided_device(poporon_t *h, uint8_t *d_data, size_t data_plane_stride,
                                                 uint8_t *d_parity, size_t parity_plane_stride, size_t size,
                                                 size_t count, const uint8_t *lost, size_t lost_count, uint8_t *d_ok,
                                                 uint8_t *d_corrected, uint8_t *d_dirty, void *stream)
{
    const PlaneCall c = {FORM_DECODE, nullptr, size, count, lost, lost_count, d_ok, d_corrected, d_dirty, {}};
    return plane_strided(h, "poporon_decode_planes_strided_device", c, d_data, data_plane_stride, d_parity,
                         parity_plane_stride, stream);
}

EXPORT bool poporon_check_planes_strided_device(poporon_t *h, const uint8_t *d_data, size_t data_plane_stride,
                                                const uint8_t *d_parity, size_t parity_plane_stride, size_t size,
                                                size_t count, uint8_t *d_dirty, void *stream)
{
    const PlaneCall c = {FORM_CHECK, nullptr, size, count, nullptr, 0, nullptr, nullptr, d_dirty, {}};
    return plane_strided(h, "poporon_check_planes_strided_device", c, d_data, data_plane_stride, d_parity,
                         parity_plane_stride, stream);
}

/* ------------------------------------------------------------------------ */
/* soft-decision decode: Chase-2 around the errors-only row decode          */
/* ------------------------------------------------------------------------ */

/*
 * A chunk of n codewords is n << flips candidate rows in the staging rows
 * (rs_soft.hip; RS_ILV_ROW bytes from one to the next, so that every row starts
 * on a 16-byte boundary and both kernels move whole uint4 slots; rows packed
 * back to back were measured and not kept), one launch_decode
 * over all of them, routed by that count, with its ok / corrected per candidate
 * in the handle's soft buffer, and the selection into the caller's arrays.  The
 * loop is its own, beside form_chunks: the
 * decode's result arrays are per candidate, not per caller codeword, and
 * nothing is gathered from or scattered to the caller's rows.  The ordering of
 * the shared buffers across streams is the staged forms'.
 */
#define SOFT_MAX_FLIPS 6u

struct SoftCall {
    const int8_t *llr;
    size_t ls;
    uint8_t *data;
    size_t ds;
    uint8_t *par;
    size_t ps;
    size_t size, count;
    unsigned flips;
    uint8_t *ok, *changed, *pattern;
    uint32_t *score;
};

static size_t soft_chunk(const poporon_t *h, unsigned flips) { return std::max<size_t>(1, h->ilv_chunk >> flips); }

static bool ensure_soft(poporon_t *h, size_t rows) { return ensure_buf(h->gpu, h->gpu.soft, rows, 2, 0); }

static bool soft_flips(const poporon_t *h, const char *what, size_t size, unsigned flips)
{
    const size_t bits = (size + h->rs->num_roots) * h->rs->gf->symbol_size;
    if (flips > SOFT_MAX_FLIPS)
        return fail("%s: flips %u > %u", what, flips, SOFT_MAX_FLIPS);
    if (flips > bits)
        return fail("%s: flips %u > the %zu bits of a codeword", what, flips, bits);
    return true;
}

/* the checks the soft call makes before it touches the GPU */
static bool soft_args(const poporon_t *h, const char *what, const SoftCall &c)
{
    if (!rs_handle(h, what) || !form_size(h, what, c.size) || !soft_flips(h, what, c.size, c.flips))
        return false;
    const size_t nr = h->rs->num_roots, bits = (c.size + nr) * h->rs->gf->symbol_size;
    if (c.ls < bits)
        return fail("%s: llr_stride %zu < (size + num_roots) * symbol_size = %zu", what, c.ls, bits);
    if (c.ds < c.size)
        return fail("%s: data_stride %zu < size %zu", what, c.ds, c.size);
    if (c.ps < nr)
        return fail("%s: parity_stride %zu < num_roots %zu", what, c.ps, nr);
    if (c.count && (!c.llr || !c.data || !c.par || !c.ok))
        return fail("%s: NULL argument", what);
    return true;
}

/* device pointers; the caller holds the batch scope and the device */
static bool soft_run(poporon_t *h, const SoftCall &c, hipStream_t s)
{
    GpuCtx &g = h->gpu;
    const uint32_t nr = h->rs->num_roots, size = (uint32_t)c.size, m = h->rs->gf->symbol_size;
    const size_t chunk = soft_chunk(h, c.flips), r0 = std::min(c.count, chunk) << c.flips;
    if (!ensure_ilv(h, r0) || !ensure_soft(h, r0) || !rem_acquire(g, s))
        return false;
    for (size_t c0 = 0; c0 < c.count; c0 += chunk) {
        const size_t n = std::min(chunk, c.count - c0);
        const int8_t *llr = c.llr + c0 * c.ls;
        STAGE(g, POPORON_AMD_KERNEL_SOFT_EXPAND, s, rsk_soft_expand(llr, c.ls, g.ilv.p, size, nr, m, c.flips, n, s));
        const DecodeCall d = {.data = g.ilv.p, .ds = RS_ILV_ROW, .par = g.ilv.p + size, .ps = RS_ILV_ROW, .size = c.size,
                              .count = n << c.flips, .ok = g.soft.p, .corrected = g.soft.p + g.soft.cap, .s = s};
        if (!launch_decode(h, d))
            return false;
        STAGE(g, POPORON_AMD_KERNEL_SOFT_SELECT, s,
              rsk_soft_select(llr, c.ls, g.ilv.p, g.soft.p, size, nr, m, c.flips, n, c.data + c0 * c.ds, c.ds,
                              c.par + c0 * c.ps, c.ps, c.ok + c0, c.changed ? c.changed + c0 : nullptr,
                              c.pattern ? c.pattern + c0 : nullptr, c.score ? c.score + c0 : nullptr, s));
    }
    return rem_release(g, s);
}

EXPORT size_t poporon_amd_soft_llr_row(const poporon_t *h, size_t size)
{
    if (!h || h->fec_type != PPLN_FEC_RS || !check_decode_size(h, size))
        return 0;
    return (size + h->rs->num_roots) * h->rs->gf->symbol_size;
}

EXPORT bool poporon_amd_reserve_soft(poporon_t *h, unsigned flips, size_t max_codewords)
{
    const char *what = "poporon_amd_reserve_soft";
    if (!rs_handle(h, what) || !soft_flips(h, what, kmax(h), flips))
        return false;
    return reserve_scope(h, what, [&] {
        const size_t rows = std::min(max_codewords, soft_chunk(h, flips)) << flips;
        return ensure_ilv(h, rows) && ensure_soft(h, rows) && ensure_rem(h, rows);
    });
}

EXPORT bool poporon_decode_soft_batch_device(poporon_t *h, const int8_t *d_llr, size_t llr_stride, uint8_t *d_data,
                                             size_t data_stride, uint8_t *d_parity, size_t parity_stride, size_t size,
                                             size_t count, unsigned flips, uint8_t *d_ok, uint8_t *d_changed,
                                             uint8_t *d_pattern, uint32_t *d_score, void *stream)
{
    const SoftCall c = {d_llr, llr_stride, d_data, data_stride, d_parity,  parity_stride, size,
                        count, flips,      d_ok,   d_changed,   d_pattern, d_score};
    return soft_args(h, "poporon_decode_soft_batch_device", c) &&
           form_scope(h, count, stream, false, [&](hipStream_t s) { return soft_run(h, c, s); });
}

/* Host form: chunks of rows through one pinned slot of its own and the device
 * form, synchronously (poporon_decode_batch's pipeline is not involved).  Slot
 * layout for n codewords:
 * [wire rows (size + nr) n | to 16 | positions nr n | counts n | ok n | corrected n | err_num n | to 16 |
 *  err_pos nr n | err_val nr n] */
static const size_t kRepHostBytes = (size_t)8 << 20;

EXPORT bool poporon_decode_batch_report(poporon_t *h, uint8_t *data, size_t data_stride, uint8_t *parity,
                                        size_t parity_stride, size_t size, size_t count, const uint8_t *positions,
                                        size_t positions_stride, const uint8_t *counts, uint8_t *ok,
                                        uint8_t *corrected, uint8_t *err_num, uint8_t *err_pos, uint8_t *err_val,
                                        size_t report_stride)
{
    const char *what = "poporon_decode_batch_report";
    const RepOut o = {err_num, err_pos, err_val, report_stride};
    if (!decode_row_args(h, what, true, data, parity, size, count, positions, positions_stride, counts, ok) ||
        !rep_args(h, what, count, o))
        return false;
    if (count == 0)
        return true;
    if (!batch_enter(h))
        return false;
    BatchScope bsc{h->gpu, nullptr, true};
    DeviceGuard dg(h->gpu.device);
    const size_t nr = h->rs->num_roots, w = size + nr;
    const size_t eb = positions ? nr : 0;
    const size_t chunk = std::max<size_t>(1, std::min(count, kRepHostBytes / (w + eb + 4 + 2 * nr)));
    auto o_pos = [&](size_t n) { return rs_ws_round16(n * w); };
    auto o_cnt = [&](size_t n) { return o_pos(n) + n * eb; };
    auto o_ok = [&](size_t n) { return o_cnt(n) + n; };
    auto o_cor = [&](size_t n) { return o_ok(n) + n; };
    auto o_num = [&](size_t n) { return o_cor(n) + n; };
    auto o_ep = [&](size_t n) { return rs_ws_round16(o_num(n) + n); };
    auto o_ev = [&](size_t n) { return o_ep(n) + n * nr; };
    return host_chunks(
        h, &h->gpu.rslot, 1, count, chunk, o_ev(chunk) + chunk * nr,
        [&](uint8_t *hb, size_t c0, size_t n) {
            copy_rows(hb, w, data + c0 * data_stride, data_stride, size, n);
            copy_rows(hb + size, w, parity + c0 * parity_stride, parity_stride, nr, n);
            if (positions) {
                copy_rows(hb + o_pos(n), nr, positions + c0 * positions_stride, positions_stride, nr, n);
                memcpy(hb + o_cnt(n), counts + c0, n);
            }
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            uint8_t *dv = ps.dev;
            HIP_OK(hipMemcpyAsync(dv, ps.host, o_ok(n), hipMemcpyHostToDevice, ps.stream));
            if (!rep_run(h, {.data = dv, .ds = w, .par = dv + size, .ps = w, .size = size, .count = n,
                             .pos8 = positions ? dv + o_pos(n) : nullptr, .pos_stride = nr, .cnt = dv + o_cnt(n),
                             .ok = dv + o_ok(n), .corrected = dv + o_cor(n), .s = ps.stream},
                         {dv + o_num(n), dv + o_ep(n), dv + o_ev(n), nr}))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host, dv, n * w, hipMemcpyDeviceToHost, ps.stream));
            HIP_OK(hipMemcpyAsync(ps.host + o_ok(n), dv + o_ok(n), o_ev(n) + n * nr - o_ok(n), hipMemcpyDeviceToHost,
                                  ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t c0, size_t n) {
            copy_rows(data + c0 * data_stride, data_stride, hb, w, size, n);
            copy_rows(parity + c0 * parity_stride, parity_stride, hb + size, w, nr, n);
            memcpy(ok + c0, hb + o_ok(n), n);
            if (corrected)
                memcpy(corrected + c0, hb + o_cor(n), n);
            memcpy(err_num + c0, hb + o_num(n), n);
            copy_rows(err_pos + c0 * report_stride, report_stride, hb + o_ep(n), nr, nr, n);
            copy_rows(err_val + c0 * report_stride, report_stride, hb + o_ev(n), nr, nr, n);
        },
        "HIP failure in a report host batch");
}

EXPORT bool poporon_amd_erasures_from_mask_device(poporon_t *h, const uint8_t *d_mask, size_t mask_stride, size_t size,
                                                  size_t depth, size_t count, uint8_t *d_positions,
                                                  size_t positions_stride, uint8_t *d_counts, uint8_t *d_over,
                                                  void *stream)
{
    const char *what = "poporon_amd_erasures_from_mask_device";
    if (!rs_handle(h, what))
        return false;
    if (count && (!d_mask || !d_positions || !d_counts))
        return fail("%s: NULL argument", what);
    if (depth < 1 || depth > RS_ILV_MAX_DEPTH)
        return fail("%s: depth %zu outside [1, %u]", what, depth, (unsigned)RS_ILV_MAX_DEPTH);
    if (!form_size(h, what, size))
        return false;
    const uint32_t nr = h->rs->num_roots;
    if (mask_stride < size * depth)
        return fail("%s: mask_stride %zu < size * depth = %zu", what, mask_stride, size * depth);
    if (positions_stride < nr)
        return fail("%s: positions_stride %zu < num_roots (%u)", what, positions_stride, (unsigned)nr);
    return form_scope(h, count, stream, false, [&](hipStream_t s) {
        const size_t step = (size_t)1 << 24; /* frames per launch: frames * depth stays below 2^31 */
        for (size_t f0 = 0; f0 < count; f0 += step) {
            const size_t n = std::min(step, count - f0), c0 = f0 * depth;
            KernelTimer t(h->gpu, POPORON_AMD_KERNEL_MASK_LISTS, s);
            HIP_OK(rsk_mask_lists(d_mask + f0 * mask_stride, mask_stride, (uint32_t)size, (uint32_t)depth, nr, n,
                                  d_positions + c0 * positions_stride, positions_stride, d_counts + c0,
                                  d_over ? d_over + c0 : nullptr, s));
            t.done();
        }
        return true;
    });
}

/* ------------------------------------------------------------------------ */
/* product-code blocks: a schedule of row passes and column passes          */
/* ------------------------------------------------------------------------ */

/*
 * A block is a codeword of the row code along every row and of the column code
 * along every column (poporon_amd.h).  poporon_product_t owns one handle per
 * axis on one device.  prod_run keeps a chunk loop of its own (two handles and
 * alternating axes are not form_chunks' loop): per chunk of whole blocks,
 * at most ilv_chunk codewords of either axis, the whole schedule is enqueued
 * -- per pass the erasure lists from the other axis's flags (rs_prod_lists_k),
 * the axis's codewords gathered into its handle's staging rows
 * (rs_product.hip), the row launchers there, routed by the chunk's count, the
 * check kernel for the pass's flags, and the rows scattered back.  Rows of a
 * block stack (bstride == n2 * pitch) are wire rows already: the row code runs
 * on the caller's buffer.  The flags live in the caller's arrays or, where it
 * passed NULL, in the object's workspace, which also holds the d_ok the row
 * decoders write.  Nothing waits for the host.
 */
struct _poporon_product_t {
    poporon_t *h[2]; /* 0: the row code, 1: the column code */
    DevBuf ws;       /* device, in bytes: [row flags n2 nb | column flags n1 nb | ok max(n1, n2) nb] of one chunk */
};

struct ProdCall {
    FormOp op;
    uint8_t *blocks;
    size_t pitch, bstride, k1, k2, count;
    int first_axis;
    size_t passes;
    int couple;
    uint8_t *row_dirty, *col_dirty, *block_ok;
};

EXPORT void poporon_amd_product_destroy(poporon_product_t *p)
{
    if (!p)
        return;
    if (p->ws.p && p->h[0] && p->h[0]->gpu.ready) {
        DeviceGuard dg(p->h[0]->gpu.device);
        (void)hipDeviceSynchronize();
        (void)hipFree(p->ws.p);
    }
    poporon_destroy(p->h[0]);
    poporon_destroy(p->h[1]);
    delete p;
}

EXPORT poporon_product_t *poporon_amd_product_create(const poporon_config_t *row_config,
                                                     const poporon_config_t *col_config)
{
    if (!row_config || !col_config) {
        fail("poporon_amd_product_create: NULL config");
        return nullptr;
    }
    if (row_config->fec_type != PPLN_FEC_RS || col_config->fec_type != PPLN_FEC_RS) {
        fail("poporon_amd_product_create serves RS configs");
        return nullptr;
    }
    if (row_config->symbol_size != col_config->symbol_size ||
        row_config->generator_polynomial != col_config->generator_polynomial) {
        fail("poporon_amd_product_create: the row code and the column code need one field (symbol_size %u / %u, "
             "polynomial 0x%X / 0x%X)",
             (unsigned)row_config->symbol_size, (unsigned)col_config->symbol_size,
             (unsigned)row_config->generator_polynomial, (unsigned)col_config->generator_polynomial);
        return nullptr;
    }
    poporon_product_t *p = new (std::nothrow) _poporon_product_t();
    if (!p)
        return nullptr;
    p->h[0] = poporon_create(row_config);
    p->h[1] = poporon_create(col_config);
    for (int a = 0; a < 2; a++) {
        if (!p->h[a] || !p->h[a]->supported) {
            poporon_amd_product_destroy(p);
            fail("poporon_amd_product_create: the %s config is not served by the GPU kernels", a ? "column" : "row");
            return nullptr;
        }
    }
    return p;
}

EXPORT poporon_t *poporon_amd_product_handle(poporon_product_t *p, int axis)
{
    return (p && (axis == 0 || axis == 1)) ? p->h[axis] : nullptr;
}

EXPORT bool poporon_amd_product_shape(const poporon_product_t *p, size_t row_size, size_t col_size, size_t *n1,
                                      size_t *n2)
{
    if (!p)
        return fail("poporon_amd_product_shape: NULL handle");
    if (!check_decode_size(p->h[0], row_size))
        return fail("poporon_amd_product_shape: row_size %zu outside [1, %u]", row_size, (unsigned)kmax(p->h[0]));
    if (!check_decode_size(p->h[1], col_size))
        return fail("poporon_amd_product_shape: col_size %zu outside [1, %u]", col_size, (unsigned)kmax(p->h[1]));
    if (n1)
        *n1 = row_size + p->h[0]->rs->num_roots;
    if (n2)
        *n2 = col_size + p->h[1]->rs->num_roots;
    return true;
}

EXPORT bool poporon_amd_product_tile(size_t codeword_bytes, size_t codewords, size_t *blocks, size_t *per_tile)
{
    uint32_t g = 0, u = 0, tpb = 0;
    if (codeword_bytes > 255 || codewords > 255 ||
        !rsk_prod_tile((uint32_t)codeword_bytes, (uint32_t)codewords, &g, &u, &tpb))
        return fail("poporon_amd_product_tile: no block of %zu codewords of %zu bytes", codewords, codeword_bytes);
    if (blocks)
        *blocks = g;
    if (per_tile)
        *per_tile = u;
    return true;
}

/* the checks every product entry point makes before it touches the GPU */
static bool prod_args(const poporon_product_t *p, const char *what, const ProdCall &c)
{
    if (!p)
        return fail("%s: NULL handle", what);
    if (!check_decode_size(p->h[0], c.k1))
        return fail("%s: row_size %zu outside [1, %u]", what, c.k1, (unsigned)kmax(p->h[0]));
    if (!check_decode_size(p->h[1], c.k2))
        return fail("%s: col_size %zu outside [1, %u]", what, c.k2, (unsigned)kmax(p->h[1]));
    const size_t n1 = c.k1 + p->h[0]->rs->num_roots, n2 = c.k2 + p->h[1]->rs->num_roots;
    if (c.pitch < n1)
        return fail("%s: row_pitch %zu < row_size + num_roots = %zu", what, c.pitch, n1);
    if (c.pitch > ((size_t)-1 - n1) / n2 || c.bstride < (n2 - 1) * c.pitch + n1)
        return fail("%s: block_stride %zu < (n2 - 1) * row_pitch + n1 = %zu", what, c.bstride,
                    (n2 - 1) * c.pitch + n1);
    if (c.op == FORM_DECODE) {
        if (c.first_axis != 0 && c.first_axis != 1)
            return fail("%s: first_axis %d is neither 0 nor 1", what, c.first_axis);
        if (c.passes < 1 || c.passes > 16)
            return fail("%s: passes %zu outside [1, 16]", what, c.passes);
    }
    if (c.op != FORM_ENCODE && !c.row_dirty && !c.col_dirty && !c.block_ok)
        return fail("%s: NULL argument (d_row_dirty, d_col_dirty and d_block_ok)", what);
    if (c.count == 0)
        return true;
    if (!c.blocks)
        return fail("%s: NULL argument (the blocks)", what);
    if (c.count > ((size_t)-1) / c.bstride)
        return fail("%s: count * block_stride passes size_t", what);
    return true;
}

/* blocks per chunk: at most ilv_chunk codewords on either axis, at least one block */
static size_t prod_chunk(const poporon_product_t *p, size_t n1, size_t n2)
{
    return std::max<size_t>(1, p->h[0]->ilv_chunk / std::max(n1, n2));
}

/* both handles' device contexts on one device, no live server beside the batch */
static bool prod_enter(poporon_product_t *p)
{
    if (!batch_enter(p->h[0]))
        return false;
    if (!p->h[1]->gpu.ready && !poporon_amd_set_device(p->h[1], p->h[0]->gpu.device)) {
        batch_exit(p->h[0]->gpu, nullptr, true);
        return false;
    }
    if (!batch_enter(p->h[1])) {
        batch_exit(p->h[0]->gpu, nullptr, true);
        return false;
    }
    return true;
}

/* the object's workspace for chunks of nb blocks; its last reader ran under both handles' rem ordering */
static bool prod_ensure_ws(poporon_product_t *p, size_t n1, size_t n2, size_t nb)
{
    const size_t need = nb * (n1 + n2 + std::max(n1, n2));
    if (p->ws.cap >= need)
        return true;
    for (int a = 0; p->ws.p && a < 2; a++) {
        GpuCtx &g = p->h[a]->gpu;
        if (g.rem_pending)
            HIP_OK(hipEventSynchronize(g.rem_done));
        g.rem_pending = false;
    }
    return buf_renew(p->ws, need, 1);
}

static bool prod_reserve(poporon_product_t *p, size_t n1, size_t n2, size_t nb)
{
    if (!prod_ensure_ws(p, n1, n2, nb))
        return false;
    const size_t cw[2] = {nb * n2, nb * n1}; /* codewords of axis a in a chunk */
    for (int a = 0; a < 2; a++)
        if (!ensure_ilv(p->h[a], cw[a]) || !ensure_rem(p->h[a], cw[a]) || !ensure_plist(p->h[a], cw[a]))
            return false;
    return true;
}

/* device pointers; the caller holds both batch scopes and the device */
static bool prod_run(poporon_product_t *p, const ProdCall &c, hipStream_t s)
{
    poporon_t *h0 = p->h[0], *h1 = p->h[1];
    const uint32_t k[2] = {(uint32_t)c.k1, (uint32_t)c.k2};
    const uint32_t r[2] = {h0->rs->num_roots, h1->rs->num_roots};
    const uint32_t n[2] = {k[0] + r[0], k[1] + r[1]}; /* n[a]: bytes of an axis-a codeword */
    const uint32_t cwn[2] = {n[1], n[0]};             /* codewords of axis a in a block */
    const size_t chunk = prod_chunk(p, n[0], n[1]), nb0 = std::min(c.count, chunk);
    const bool inplace = c.bstride == (size_t)n[1] * c.pitch; /* the blocks' rows are wire rows at stride pitch */
    if (!prod_ensure_ws(p, n[0], n[1], nb0))
        return false;
    if (!ensure_ilv(h1, nb0 * n[0]) || ((!inplace) && !ensure_ilv(h0, nb0 * n[1])))
        return false;
    if (c.op == FORM_DECODE && c.couple) /* passes 1, 2, ... take lists: the second axis, then the first again */
        for (size_t pass = 1; pass < std::min<size_t>(c.passes, 3); pass++) {
            const int a = (c.first_axis + (int)pass) & 1;
            if (!ensure_plist(p->h[a], nb0 * cwn[a]))
                return false;
        }
    if (!rem_acquire(h0->gpu, s) || !rem_acquire(h1->gpu, s))
        return false;
    for (size_t b0 = 0; b0 < c.count; b0 += chunk) {
        const size_t nb = std::min(chunk, c.count - b0);
        uint8_t *blk = c.blocks + b0 * c.bstride;
        uint8_t *flag[2] = {c.row_dirty ? c.row_dirty + b0 * n[1] : p->ws.p,
                            c.col_dirty ? c.col_dirty + b0 * n[0] : p->ws.p + nb0 * n[1]};
        uint8_t *okbuf = p->ws.p + nb0 * (n[0] + n[1]);
        /* axis a's codewords of the chunk as rows: where they are, gathered first unless they are the block rows */
        auto stage = [&](int a, uint32_t cw, uint32_t m1, uint8_t *&data, size_t &ds) -> bool {
            poporon_t *h = p->h[a];
            if (a == 0 && inplace) {
                data = blk;
                ds = c.pitch;
                return true;
            }
            data = h->gpu.ilv.p;
            ds = n[a];
            STAGE(h->gpu, POPORON_AMD_KERNEL_PROD_GATHER, s,
                  rsk_prod_gather(blk, c.pitch, c.bstride, nb, (uint32_t)a, n[a], cw, 0u, m1, data, s));
            return true;
        };
        auto unstage = [&](int a, uint32_t cw, uint32_t m0) -> bool {
            poporon_t *h = p->h[a];
            if (a == 0 && inplace)
                return true;
            STAGE(h->gpu, POPORON_AMD_KERNEL_PROD_SCATTER, s,
                  rsk_prod_scatter(h->gpu.ilv.p, blk, c.pitch, c.bstride, nb, (uint32_t)a, n[a], cw, m0, n[a], s));
            return true;
        };
        auto check = [&](int a) -> bool {
            uint8_t *data;
            size_t ds;
            return stage(a, cwn[a], n[a], data, ds) &&
                   launch_check(p->h[a], data, ds, data + k[a], ds, k[a], nb * cwn[a], flag[a], s);
        };
        if (c.op == FORM_ENCODE) {
            /* column parity of the message columns, then row parity of every row: the checks on checks come out
             * the same either way round (one field) */
            for (int a = 1; a >= 0; a--) {
                const uint32_t cw = a ? k[0] : n[1];
                uint8_t *data;
                size_t ds;
                if (!stage(a, cw, k[a], data, ds) ||
                    !launch_encode(p->h[a], data, ds, data + k[a], ds, k[a], nb * cw, s) || !unstage(a, cw, k[a]))
                    return false;
            }
            continue;
        }
        if (c.op == FORM_CHECK) {
            if (!check(0) || !check(1))
                return false;
        } else {
            int a = c.first_axis;
            for (size_t pass = 0; pass < c.passes; pass++, a ^= 1) {
                poporon_t *h = p->h[a];
                GpuCtx &g = h->gpu;
                const size_t ls = plane_list_stride(h), ncw = nb * cwn[a];
                const bool lists = c.couple && pass > 0;
                if (lists)
                    STAGE(g, POPORON_AMD_KERNEL_PROD_LISTS, s,
                          rsk_prod_lists(flag[a ^ 1], n[a], r[a], cwn[a], g.plist.p, (uint32_t)ls,
                                         g.plist.p + g.plist.cap * ls, nb, s));
                uint8_t *data;
                size_t ds;
                if (!stage(a, cwn[a], n[a], data, ds))
                    return false;
                const DecodeCall d = {.data = data, .ds = ds, .par = data + k[a], .ps = ds, .size = k[a], .count = ncw,
                                      .pos8 = lists ? g.plist.p : nullptr, .pos_stride = ls,
                                      .cnt = lists ? g.plist.p + g.plist.cap * ls : nullptr, .ok = okbuf,
                                      .corrected = nullptr, .s = s};
                if (!launch_decode(h, d) || !launch_check(h, data, ds, data + k[a], ds, k[a], ncw, flag[a], s) ||
                    !unstage(a, cwn[a], 0u))
                    return false;
            }
            if (!check(a)) /* the axis the last pass did not run on, on the block as returned */
                return false;
        }
        if (c.block_ok)
            STAGE(h0->gpu, POPORON_AMD_KERNEL_PROD_LISTS, s,
                  rsk_prod_ok(flag[0], n[1], flag[1], n[0], c.block_ok + b0, nb, s));
    }
    return rem_release(h0->gpu, s) && rem_release(h1->gpu, s);
}

/* form_scope over both handles */
template <class F> static bool prod_scope(poporon_product_t *p, size_t count, void *stream, bool host, F &&run)
{
    if (count == 0)
        return true;
    if (!prod_enter(p))
        return false;
    BatchScope bs0{p->h[0]->gpu, (hipStream_t)stream, host}, bs1{p->h[1]->gpu, (hipStream_t)stream, host};
    DeviceGuard dg(p->h[0]->gpu.device);
    return run((hipStream_t)stream);
}

static bool prod_device(poporon_product_t *p, const char *what, const ProdCall &c, void *stream)
{
    return prod_args(p, what, c) &&
           prod_scope(p, c.count, stream, false, [&](hipStream_t s) { return prod_run(p, c, s); });
}

EXPORT bool poporon_amd_product_reserve(poporon_product_t *p, size_t row_size, size_t col_size, size_t max_blocks)
{
    size_t n1 = 0, n2 = 0;
    if (!p)
        return fail("poporon_amd_product_reserve: NULL handle");
    if (!poporon_amd_product_shape(p, row_size, col_size, &n1, &n2))
        return false;
    if (!gpu_init(p->h[0]) || (!p->h[1]->gpu.ready && !poporon_amd_set_device(p->h[1], p->h[0]->gpu.device)) ||
        !gpu_init(p->h[1]))
        return false;
    DeviceGuard dg(p->h[0]->gpu.device);
    return prod_reserve(p, n1, n2, std::max<size_t>(1, std::min(max_blocks, prod_chunk(p, n1, n2))));
}

EXPORT bool poporon_encode_product_device(poporon_product_t *p, uint8_t *d_blocks, size_t row_pitch,
                                          size_t block_stride, size_t row_size, size_t col_size, size_t count,
                                          void *stream)
{
    const ProdCall c = {FORM_ENCODE, d_blocks, row_pitch, block_stride, row_size, col_size, count, 0, 0, 0,
                        nullptr,     nullptr,  nullptr};
    return prod_device(p, "poporon_encode_product_device", c, stream);
}

EXPORT bool poporon_decode_product_device(poporon_product_t *p, uint8_t *d_blocks, size_t row_pitch,
                                          size_t block_stride, size_t row_size, size_t col_size, size_t count,
                                          int first_axis, size_t passes, int couple, uint8_t *d_row_dirty,
                                          uint8_t *d_col_dirty, uint8_t *d_block_ok, void *stream)
{
    const ProdCall c = {FORM_DECODE, d_blocks, row_pitch, block_stride, row_size,    col_size,   count,
                        first_axis,  passes,   couple,    d_row_dirty,  d_col_dirty, d_block_ok};
    return prod_device(p, "poporon_decode_product_device", c, stream);
}

EXPORT bool poporon_check_product_device(poporon_product_t *p, const uint8_t *d_blocks, size_t row_pitch,
                                         size_t block_stride, size_t row_size, size_t col_size, size_t count,
                                         uint8_t *d_row_dirty, uint8_t *d_col_dirty, uint8_t *d_block_ok, void *stream)
{
    const ProdCall c = {FORM_CHECK, const_cast<uint8_t *>(d_blocks), row_pitch, block_stride, row_size, col_size,
                        count,      0, 0, 0, d_row_dirty, d_col_dirty, d_block_ok};
    return prod_device(p, "poporon_check_product_device", c, stream);
}

/* Host forms: chunks of blocks through the row handle's first pinned slot and the device form, synchronously.
 * Slot layout for n blocks, packed (pitch n1, stride n1 n2: the in-place row route):
 * [blocks n1 n2 n | row flags n2 n | column flags n1 n | block ok n] */
static const size_t kProdHostBytes = (size_t)8 << 20;

static bool prod_host_run(poporon_product_t *p, const ProdCall &c)
{
    const size_t n1 = c.k1 + p->h[0]->rs->num_roots, n2 = c.k2 + p->h[1]->rs->num_roots, bb = n1 * n2;
    const size_t chunk = std::max<size_t>(1, std::min(c.count, kProdHostBytes / (bb + n1 + n2 + 1)));
    const bool enc = c.op == FORM_ENCODE;
    auto o_row = [&](size_t n) { return n * bb; };
    auto o_col = [&](size_t n) { return o_row(n) + n * n2; };
    auto o_ok = [&](size_t n) { return o_col(n) + n * n1; };
    return host_chunks(
        p->h[0], &p->h[0]->gpu.pipe[0], 1, c.count, chunk, o_ok(chunk) + chunk,
        [&](uint8_t *hb, size_t b0, size_t n) {
            /* an encode reads the message rectangle only */
            const size_t rows = enc ? c.k2 : n2, cols = enc ? c.k1 : n1;
            for (size_t b = 0; b < n; b++)
                for (size_t i = 0; i < rows; i++)
                    memcpy(hb + b * bb + i * n1, c.blocks + (b0 + b) * c.bstride + i * c.pitch, cols);
        },
        [&](GpuCtx::PipeSlot &ps, size_t n) {
            ProdCall d = c;
            d.blocks = ps.dev;
            d.pitch = n1;
            d.bstride = bb;
            d.count = n;
            d.row_dirty = ps.dev + o_row(n);
            d.col_dirty = ps.dev + o_col(n);
            d.block_ok = ps.dev + o_ok(n);
            HIP_OK(hipMemcpyAsync(ps.dev, ps.host, n * bb, hipMemcpyHostToDevice, ps.stream));
            if (!prod_run(p, d, ps.stream))
                return false;
            HIP_OK(hipMemcpyAsync(ps.host, ps.dev, enc ? n * bb : o_ok(n) + n, hipMemcpyDeviceToHost, ps.stream));
            return true;
        },
        [&](const uint8_t *hb, size_t b0, size_t n) {
            for (size_t b = 0; b < n; b++)
                for (size_t i = 0; i < n2; i++) {
                    /* an encode hands back parity only: the tail of a message row, the whole of a parity row */
                    const size_t j0 = enc && i < c.k2 ? c.k1 : 0;
                    memcpy(c.blocks + (b0 + b) * c.bstride + i * c.pitch + j0, hb + b * bb + i * n1 + j0, n1 - j0);
                }
            if (enc)
                return;
            if (c.row_dirty)
                memcpy(c.row_dirty + b0 * n2, hb + o_row(n), n * n2);
            if (c.col_dirty)
                memcpy(c.col_dirty + b0 * n1, hb + o_col(n), n * n1);
            if (c.block_ok)
                memcpy(c.block_ok + b0, hb + o_ok(n), n);
        },
        "HIP failure in a product-code host batch");
}

static bool prod_host(poporon_product_t *p, const char *what, const ProdCall &c)
{
    return prod_args(p, what, c) &&
           prod_scope(p, c.count, nullptr, true, [&](hipStream_t) { return prod_host_run(p, c); });
}

EXPORT bool poporon_encode_product(poporon_product_t *p, uint8_t *blocks, size_t row_pitch, size_t block_stride,
                                   size_t row_size, size_t col_size, size_t count)
{
    const ProdCall c = {FORM_ENCODE, blocks, row_pitch, block_stride, row_size, col_size, count, 0, 0, 0,
                        nullptr,     nullptr, nullptr};
    return prod_host(p, "poporon_encode_product", c);
}

EXPORT bool poporon_decode_product(poporon_product_t *p, uint8_t *blocks, size_t row_pitch, size_t block_stride,
                                   size_t row_size, size_t col_size, size_t count, int first_axis, size_t passes,
                                   int couple, uint8_t *row_dirty, uint8_t *col_dirty, uint8_t *block_ok)
{
    const ProdCall c = {FORM_DECODE, blocks, row_pitch, block_stride, row_size,  col_size, count,
                        first_axis,  passes, couple,    row_dirty,    col_dirty, block_ok};
    return prod_host(p, "poporon_decode_product", c);
}

/* ------------------------------------------------------------------------ */
/* K = 7 convolutional code: batch encode and blocked Viterbi decode        */
/* ------------------------------------------------------------------------ */

/*
 * The handle is the code's parameters and nothing else (cc.hip takes them by
 * value): no device memory, no streams, no timing.  A decode is count * blocks
 * waves, an encode count * words threads; either goes out in launches of at
 * most cc->chunk blocks (64 cc->chunk encode threads), one after another on the
 * caller's stream, on the current device.
 */
/* the fastest setting of tools/cc_bench.py whose errors at rate 7/8 stay inside the seed-to-seed spread of the
 * overlap = 1024 column */
#define CC_BLOCK_DEFAULT 512u
#define CC_OVERLAP_DEFAULT 96u
#define CC_CHUNK_DEFAULT ((size_t)1 << 22)
#define CC_CHUNK_MAX ((size_t)1 << 24)

struct _poporon_cc_t {
    CcParams p;
    size_t chunk; /* decode blocks per launch (POPORON_AMD_CC_CHUNK) */
};

EXPORT poporon_cc_t *poporon_amd_cc_create(unsigned g0, unsigned g1, unsigned invert, unsigned period, uint32_t keep0,
                                           uint32_t keep1, unsigned block, unsigned overlap)
{
    const char *what = "poporon_amd_cc_create";
    if (block == 0u)
        block = CC_BLOCK_DEFAULT;
    if (overlap == 0xFFFFFFFFu)
        overlap = CC_OVERLAP_DEFAULT;
    bool ok = true;
    if (g0 < 1u || g0 > 127u || g1 < 1u || g1 > 127u)
        ok = fail("%s: polynomials %#o, %#o outside [1, 0177]", what, g0, g1);
    else if (invert > 3u)
        ok = fail("%s: invert %u > 3", what, invert);
    else if (period < 1u || period > CC_PERIOD_MAX)
        ok = fail("%s: period %u outside [1, %u]", what, period, CC_PERIOD_MAX);
    else if ((keep0 | keep1) >> period)
        ok = fail("%s: a puncture mask (%#x, %#x) has a bit at or above the period %u", what, keep0, keep1, period);
    else if (!(keep0 | keep1))
        ok = fail("%s: the puncture masks keep nothing", what);
    else if (block % 64u || block < 64u || block > CC_BLOCK_MAX)
        ok = fail("%s: block %u is no multiple of 64 in [64, %u]", what, block, CC_BLOCK_MAX);
    else if (overlap > CC_OVERLAP_MAX)
        ok = fail("%s: overlap %u > %u", what, overlap, CC_OVERLAP_MAX);
    if (!ok)
        return nullptr;
    poporon_cc_t *cc = new (std::nothrow) poporon_cc_t();
    if (!cc) {
        fail("%s: out of memory", what);
        return nullptr;
    }
    cc->p = {g0, g1, invert, period, keep0, keep1,
             (uint32_t)(__builtin_popcount(keep0) + __builtin_popcount(keep1)), block, overlap};
    const char *ch = getenv("POPORON_AMD_CC_CHUNK");
    const unsigned long long v = ch ? strtoull(ch, nullptr, 10) : 0ull;
    cc->chunk = v ? (size_t)std::min<unsigned long long>(v, CC_CHUNK_MAX) : CC_CHUNK_DEFAULT;
    return cc;
}

EXPORT void poporon_amd_cc_destroy(poporon_cc_t *cc) { delete cc; }

EXPORT size_t poporon_amd_cc_symbols(const poporon_cc_t *cc, size_t nbits)
{
    return cc ? (size_t)cc_symbols_before(cc->p, nbits) : 0;
}

EXPORT size_t poporon_amd_cc_blocks(const poporon_cc_t *cc, size_t nbits)
{
    return cc ? nbits / cc->p.block + (nbits % cc->p.block != 0) : 0;
}

EXPORT bool poporon_cc_encode_device(const poporon_cc_t *cc, const uint8_t *d_bits, size_t bits_stride, size_t nbits,
                                     size_t count, int start_state, uint8_t *d_symbols, size_t symbols_stride,
                                     uint8_t *d_end_state, void *stream)
{
    const char *what = "poporon_cc_encode_device";
    if (!cc)
        return fail("%s: NULL handle", what);
    if (nbits == 0)
        return fail("%s: nbits is 0", what);
    if (start_state < 0 || start_state > 63)
        return fail("%s: start_state %d outside [0, 63]", what, start_state);
    const size_t m = poporon_amd_cc_symbols(cc, nbits), fb = nbits / 8 + (nbits % 8 != 0), sb = m / 8 + (m % 8 != 0);
    if (bits_stride < fb)
        return fail("%s: bits_stride %zu < the %zu bytes of a frame", what, bits_stride, fb);
    if (symbols_stride < sb)
        return fail("%s: symbols_stride %zu < the %zu bytes of a frame's symbols", what, symbols_stride, sb);
    if (count == 0)
        return true;
    if (!d_bits || !d_symbols)
        return fail("%s: NULL argument", what);
    const uint64_t words = std::max<uint64_t>(1, m / 32 + (m % 32 != 0)), total = words * count;
    const uint64_t per = (uint64_t)cc->chunk * CC_STATES;
    for (uint64_t first = 0; first < total; first += per)
        HIP_OK(cck_encode(&cc->p, d_bits, bits_stride, nbits, m, words, first, std::min(per, total - first), start_state,
                          d_symbols, symbols_stride, d_end_state, static_cast<hipStream_t>(stream)));
    return true;
}

EXPORT bool poporon_cc_decode_device(const poporon_cc_t *cc, const int8_t *d_llr, size_t llr_stride, size_t nbits,
                                     size_t count, int start_state, int end_state, uint8_t *d_bits, size_t bits_stride,
                                     uint32_t *d_metric, void *stream)
{
    const char *what = "poporon_cc_decode_device";
    if (!cc)
        return fail("%s: NULL handle", what);
    if (nbits == 0)
        return fail("%s: nbits is 0", what);
    if (start_state < -1 || start_state > 63)
        return fail("%s: start_state %d outside [-1, 63]", what, start_state);
    if (end_state < -1 || end_state > 63)
        return fail("%s: end_state %d outside [-1, 63]", what, end_state);
    const size_t m = poporon_amd_cc_symbols(cc, nbits), fb = nbits / 8 + (nbits % 8 != 0);
    if (llr_stride < m)
        return fail("%s: llr_stride %zu < the %zu symbols of a frame", what, llr_stride, m);
    if (bits_stride < fb)
        return fail("%s: bits_stride %zu < the %zu bytes of a frame", what, bits_stride, fb);
    if (count == 0)
        return true;
    if (!d_llr || !d_bits)
        return fail("%s: NULL argument", what);
    const uint64_t blocks = poporon_amd_cc_blocks(cc, nbits), total = blocks * count;
    for (uint64_t first = 0; first < total; first += cc->chunk)
        HIP_OK(cck_decode(&cc->p, d_llr, llr_stride, nbits, blocks, first,
                          (uint32_t)std::min<uint64_t>(cc->chunk, total - first), start_state, end_state, d_bits,
                          bits_stride, d_metric, static_cast<hipStream_t>(stream)));
    return true;
}

EXPORT bool poporon_cc_decode_siso_device(const poporon_cc_t *cc, const int8_t *d_llr, size_t llr_stride, size_t nbits,
                                          size_t count, int start_state, int end_state, unsigned shift, int8_t *d_soft,
                                          size_t soft_stride, void *stream)
{
    const char *what = "poporon_cc_decode_siso_device";
    if (!cc)
        return fail("%s: NULL handle", what);
    if (nbits == 0)
        return fail("%s: nbits is 0", what);
    if (start_state < -1 || start_state > 63)
        return fail("%s: start_state %d outside [-1, 63]", what, start_state);
    if (end_state < -1 || end_state > 63)
        return fail("%s: end_state %d outside [-1, 63]", what, end_state);
    if (shift > 8u)
        return fail("%s: shift %u > 8", what, shift);
    const size_t m = poporon_amd_cc_symbols(cc, nbits);
    if (llr_stride < m)
        return fail("%s: llr_stride %zu < the %zu symbols of a frame", what, llr_stride, m);
    if (soft_stride < nbits)
        return fail("%s: soft_stride %zu < the %zu bytes of a frame", what, soft_stride, nbits);
    if (count == 0)
        return true;
    if (!d_llr || !d_soft)
        return fail("%s: NULL argument", what);
    const uint64_t blocks = poporon_amd_cc_blocks(cc, nbits), total = blocks * count;
    for (uint64_t first = 0; first < total; first += cc->chunk)
        HIP_OK(cck_decode_soft(&cc->p, d_llr, llr_stride, nbits, blocks, first,
                               (uint32_t)std::min<uint64_t>(cc->chunk, total - first), start_state, end_state, shift,
                               d_soft, soft_stride, static_cast<hipStream_t>(stream)));
    return true;
}

/* ------------------------------------------------------------------------ */
/* multi-GPU: one handle per device, contiguous codeword ranges             */
/* ------------------------------------------------------------------------ */

/*
 * Codewords are independent: a batch is split into
 * contiguous ranges, device i taking [count*i/G, count*(i+1)/G), and no data
 * crosses between devices.  Each device has its own handle (tables,
 * workspace, streams); the host entry points run one host thread per device,
 * each driving its handle's pinned pipeline over its range, so the devices'
 * PCIe links and kernels work concurrently.
 */
struct _poporon_multi_t {
    std::vector<poporon_t *> h;
};

EXPORT bool poporon_amd_multi_range(size_t count, size_t parts, size_t part, size_t *first, size_t *n)
{
    if (parts == 0 || part >= parts || !first || !n)
        return fail("bad partition arguments");
    /* 128-bit products: count * part may exceed 64 bits for huge counts */
    const size_t a = (size_t)(((unsigned __int128)count * part) / parts);
    const size_t b = (size_t)(((unsigned __int128)count * (part + 1)) / parts);
    *first = a;
    *n = b - a;
    return true;
}

EXPORT void poporon_amd_multi_destroy(poporon_multi_t *m)
{
    if (!m)
        return;
    for (auto *p : m->h)
        poporon_destroy(p);
    delete m;
}

EXPORT poporon_multi_t *poporon_amd_multi_create(const poporon_config_t *config, const int *devices,
                                                 size_t num_devices)
{
    if (!config)
        return nullptr;
    if (config->fec_type != PPLN_FEC_RS && config->fec_type != PPLN_FEC_BCH) {
        fail("the multi-GPU handle serves RS and BCH configs");
        return nullptr;
    }
    std::vector<int> devs;
    if (devices) {
        devs.assign(devices, devices + num_devices);
    } else {
        const int n = poporon_amd_device_count();
        for (int d = 0; d < n; d++)
            devs.push_back(d);
    }
    if (devs.empty()) {
        fail("no HIP device for the multi-GPU handle");
        return nullptr;
    }
    poporon_multi_t *m = new (std::nothrow) _poporon_multi_t();
    if (!m)
        return nullptr;
    /* a device may be listed more than once: its handles are independent
     * (own tables, workspace, streams and host threads) and share that GPU --
     * e.g. two host pipelines per device, or the G > 1 split exercised on a
     * one-GPU machine (tests/test_gpu_fullsize.py) */
    for (size_t i = 0; i < devs.size(); i++) {
        poporon_t *p = poporon_create(config);
        if (!p || !poporon_amd_set_device(p, devs[i]) || !gpu_init(p)) {
            const std::string msg = g_last_error;
            poporon_destroy(p);
            poporon_amd_multi_destroy(m);
            fail("device %d: %s", devs[i], msg.c_str());
            return nullptr;
        }
        m->h.push_back(p);
    }
    return m;
}

EXPORT size_t poporon_amd_multi_device_count(const poporon_multi_t *m) { return m ? m->h.size() : 0; }

EXPORT poporon_t *poporon_amd_multi_handle(poporon_multi_t *m, size_t index)
{
    return (m && index < m->h.size()) ? m->h[index] : nullptr;
}

/* run f(i, first, n) for every device's range, one host thread per device;
 * the first failure's message is kept */
template <class F>
static bool multi_run(poporon_multi_t *m, size_t count, F &&f)
{
    const size_t G = m->h.size();
    std::vector<std::string> err(G);
    std::vector<char> okv(G, 1);
    std::vector<std::thread> th;
    auto one = [&](size_t i) {
        size_t first = 0, n = 0;
        poporon_amd_multi_range(count, G, i, &first, &n);
        if (n && !f(i, first, n)) {
            okv[i] = 0;
            err[i] = g_last_error;
        }
    };
    for (size_t i = 1; i < G; i++)
        th.emplace_back(one, i);
    one(0);
    for (auto &t : th)
        t.join();
    for (size_t i = 0; i < G; i++)
        if (!okv[i])
            return fail("device %zu: %s", i, err[i].c_str());
    return true;
}

EXPORT bool poporon_encode_batch_multi(poporon_multi_t *m, const uint8_t *data, size_t data_stride, uint8_t *parity,
                                       size_t parity_stride, size_t size, size_t count)
{
    if (!m || (count && (!data || !parity)))
        return fail("NULL argument");
    return multi_run(m, count, [&](size_t i, size_t c0, size_t n) {
        return poporon_encode_batch(m->h[i], data + c0 * data_stride, data_stride, parity + c0 * parity_stride,
                                    parity_stride, size, n);
    });
}

EXPORT bool poporon_decode_batch_multi(poporon_multi_t *m, uint8_t *data, size_t data_stride, uint8_t *parity,
                                       size_t parity_stride, size_t size, size_t count, const uint8_t *positions,
                                       size_t positions_stride, const uint8_t *counts, uint8_t *ok,
                                       uint8_t *corrected)
{
    if (!m || (count && (!data || !parity || !ok)))
        return fail("NULL argument");
    return multi_run(m, count, [&](size_t i, size_t c0, size_t n) {
        return poporon_decode_batch(m->h[i], data + c0 * data_stride, data_stride, parity + c0 * parity_stride,
                                    parity_stride, size, n, positions ? positions + c0 * positions_stride : nullptr,
                                    positions_stride, counts ? counts + c0 : nullptr, ok + c0,
                                    corrected ? corrected + c0 : nullptr);
    });
}

/* Device-resident shards: device i's range (poporon_amd_multi_range) sits at
 * the i-th pointer of each array, in that device's memory; enqueued on
 * streams[i] (streams may be NULL: each device's null stream).  Returns once
 * every device's work is enqueued. */
EXPORT bool poporon_encode_batch_multi_device(poporon_multi_t *m, const uint8_t *const *d_data, size_t data_stride,
                                              uint8_t *const *d_parity, size_t parity_stride, size_t size,
                                              size_t count, void *const *streams)
{
    if (!m || (count && (!d_data || !d_parity)))
        return fail("NULL argument");
    return multi_run(m, count, [&](size_t i, size_t, size_t n) {
        return poporon_encode_batch_device(m->h[i], d_data[i], data_stride, d_parity[i], parity_stride, size, n,
                                           streams ? streams[i] : nullptr);
    });
}

EXPORT bool poporon_decode_batch_multi_device(poporon_multi_t *m, uint8_t *const *d_data, size_t data_stride,
                                              uint8_t *const *d_parity, size_t parity_stride, size_t size,
                                              size_t count, const uint8_t *const *d_positions,
                                              size_t positions_stride, const uint8_t *const *d_counts,
                                              uint8_t *const *d_ok, uint8_t *const *d_corrected, void *const *streams)
{
    if (!m || (count && (!d_data || !d_parity || !d_ok)))
        return fail("NULL argument");
    return multi_run(m, count, [&](size_t i, size_t, size_t n) {
        return poporon_decode_batch_device(m->h[i], d_data[i], data_stride, d_parity[i], parity_stride, size, n,
                                           d_positions ? d_positions[i] : nullptr, positions_stride,
                                           d_counts ? d_counts[i] : nullptr, d_ok[i],
                                           d_corrected ? d_corrected[i] : nullptr, streams ? streams[i] : nullptr);
    });
}

/* ------------------------------------------------------------------------ */
/* single-codeword API (the reference's entry points): a batch of one       */
/* ------------------------------------------------------------------------ */

/* the coherent host buffer of the single-call paths (GpuCtx::zc, layout
 * ZC_* in rs_device.h); false if the device cannot address it (then the copy
 * paths run) */
static bool ensure_zc(GpuCtx &g)
{
    if (!g.zc) {
        void *dp = nullptr;
        uint8_t *hp = nullptr;
        if (hipHostMalloc((void **)&hp, ZC_BYTES, hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
            memset(hp, 0, ZC_BYTES);
            g.zc_dev = (uint8_t *)dp;
        } else {
            (void)hipGetLastError();
        }
        if (hp) { /* published under the registry lock: yield_servers writes other handles' buffers */
            if (g.registered) {
                std::lock_guard<std::mutex> lk(g_devs[g.device].mu);
                g.zc = hp;
            } else {
                g.zc = hp;
            }
        }
    }
    return g.zc_dev != nullptr;
}

/* Next completion word of a single-call launch (never 0), with ZC_FLAG
 * cleared first: the server answers with request words from its own counter
 * (srv_seq), so the word it left there could equal the next zc_seq and
 * zc_wait would return before this launch wrote anything */
static uint32_t zc_arm(GpuCtx &g)
{
    *reinterpret_cast<volatile uint32_t *>(g.zc + ZC_FLAG) = 0u;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    uint32_t s = ++g.zc_seq;
    if (s == 0u)
        s = ++g.zc_seq;
    return s;
}

/* Wait for a single-call kernel's completion word (it stores `seq` at
 * ZC_FLAG with a system-scope release after every result): polling host
 * memory costs the caller ~1 us after the kernel ends, a stream
 * synchronisation several.  The stream is queried now and then so that a
 * failed launch cannot leave the caller spinning. */
static bool zc_wait(GpuCtx &g, uint32_t seq)
{
    const volatile uint32_t *f = reinterpret_cast<const volatile uint32_t *>(g.zc + ZC_FLAG);
    for (uint32_t spin = 1;; ++spin) {
        if (*f == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
        if ((spin & 4095u) == 0u) {
            const hipError_t e = hipStreamQuery(g.stream);
            if (e == hipSuccess) {
                if (*f == seq) {
                    std::atomic_thread_fence(std::memory_order_acquire);
                    return true;
                }
                return fail("single-codeword kernel ended without its completion word");
            }
            if (e != hipErrorNotReady)
                return fail("HIP error %d (%s) in a single-codeword call", (int)e, hipGetErrorString(e));
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

/* The single-call server (rs_serve_k, rs_single.hip): a resident workgroup
 * that polls the handle's coherent buffer, so a poporon_encode /
 * poporon_decode call is a few posted PCIe writes and reads instead of a
 * kernel launch.  It leaves by itself after SRV_IDLE_TICKS without a request
 * (so a stream or device synchronisation waits at most that long for it) or
 * SRV_MAX_TICKS in all; the next call then launches it again.
 * POPORON_AMD_SERVE=0 turns it off (one launch per call, rs_enc1_k /
 * rs_dec1_k). */
#define SRV_IDLE_TICKS 100000ull  /* 1 ms of s_memrealtime (100 MHz) */
#define SRV_MAX_TICKS 50000000ull /* 0.5 s */

static bool serve_enabled()
{
    static const bool on = [] {
        const char *e = getenv("POPORON_AMD_SERVE");
        return !(e && e[0] == '0');
    }();
    return on;
}

/* Launch a server for the handle unless a batch of another handle on the
 * device may still be running (then -1: the caller serves this request with
 * one launch); 1 launched, 0 error.  Under the registry lock, so that a
 * batch_enter either sees this server (and bumps its yield word) or is seen
 * here. */
static int srv_launch(poporon_t *h, uint32_t last)
{
    GpuCtx &g = h->gpu;
    if (!g.sstream)
        HIP_OK(hipStreamCreateWithFlags(&g.sstream, hipStreamNonBlocking));
    std::unique_lock<std::mutex> lk;
    if (g.registered)
        lk = std::unique_lock<std::mutex>(g_devs[g.device].mu);
    if (g.registered)
        for (GpuCtx *x : g_devs[g.device].ctx) {
            if (x == &g)
                continue;
            if (x->batch_open)
                return -1;
            if (x->batch_ev_live) {
                const hipError_t q = hipEventQuery(x->batch_ev);
                if (q == hipErrorNotReady)
                    return -1;
                x->batch_ev_live = false;
            }
        }
    const uint32_t yv = *reinterpret_cast<volatile uint32_t *>(g.zc + ZC_YIELD);
    const uint32_t id = g.srv_id + 1u;
    if (h->fast || h->nrsplit) {
        RsCorrParams prm = h->corr;
        HIP_OK(rsk_serve(g.tab, &prm, g.zc_dev, last, id, yv, SRV_IDLE_TICKS, SRV_MAX_TICKS, g.sstream));
    } else { /* general parameters: one wave, GZ_* payload (rs_generic.hip rsgw_serve_k) */
        RsGenParams prm = h->gen;
        HIP_OK(rsgw_serve(g.gtab, &prm, g.zc_dev, last, id, yv, SRV_IDLE_TICKS, SRV_MAX_TICKS, g.sstream));
    }
    g.srv_id = id;
    g.srv_on = true;
    return 1;
}

/* One request through the server; the payload is in g.zc already.  A server
 * that left before it saw the request (idle limit, lifetime, yield) has
 * stored its id to ZC_EXITED without serving it: launch a new one for it.
 * 1 served, 0 error, -1 not served (another handle's batch may be running,
 * srv_launch): the caller launches the request's kernel instead. */
static int srv_call(poporon_t *h, uint32_t op, uint32_t size, uint32_t mode)
{
    GpuCtx &g = h->gpu;
    volatile uint32_t *z32 = reinterpret_cast<volatile uint32_t *>(g.zc);
    /* the request word differs from the last one the server saw */
    const uint32_t prev = z32[ZC_REQ / 4], word = srv_word(g, prev, op, size, mode);
    z32[ZC_FLAG / 4] = 0u; /* the server answers with the request word (never 0: op >= 1) */
    std::atomic_thread_fence(std::memory_order_release); /* the payload before the request word */
    z32[ZC_REQ / 4] = word;
    if (!g.srv_on) {
        const int l = srv_launch(h, prev);
        if (l <= 0)
            return l; /* the request word stays unserved: the next server starts past it */
    }
    const volatile uint32_t *f = z32 + ZC_FLAG / 4, *ex = z32 + ZC_EXITED / 4;
    for (uint32_t spin = 1;; ++spin) {
        if (*f == word) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
        if (*ex == g.srv_id) { /* the server has left */
            std::atomic_thread_fence(std::memory_order_acquire);
            if (*f == word) {
                std::atomic_thread_fence(std::memory_order_acquire);
                return true;
            }
            g.srv_on = false;
            const int l = srv_launch(h, prev);
            if (l <= 0)
                return l;
            continue;
        }
        if ((spin & 4095u) == 0u) {
            const hipError_t e = hipStreamQuery(g.sstream);
            if (e == hipSuccess && *ex != g.srv_id && *f != word) {
                g.srv_on = false;
                return fail("single-call server ended without serving or leaving its exit word");
            }
            if (e != hipSuccess && e != hipErrorNotReady) {
                g.srv_on = false;
                return fail("HIP error %d (%s) in the single-call server", (int)e, hipGetErrorString(e));
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

/* A live server of this handle leaves now (a stop request, then its exit
 * word: one PCIe round trip).  Batch calls come here first (batch_enter): a
 * resident server holds one CU's LDS, so one workgroup of a persistent batch
 * grid would wait for its idle limit, and with GPU_MAX_HW_QUEUES below the
 * streams in use its dispatch can share a hardware queue with the batch's.
 * The next single call launches a new server. */
#define SRV_STOP_DEADLINE_S 10
static bool srv_stop(poporon_t *h)
{
    GpuCtx &g = h->gpu;
    if (!g.srv_on || !g.zc)
        return true;
    volatile uint32_t *z32 = reinterpret_cast<volatile uint32_t *>(g.zc);
    const uint32_t prev = z32[ZC_REQ / 4];
    std::atomic_thread_fence(std::memory_order_release);
    z32[ZC_REQ / 4] = srv_word(g, prev, RS_SRV_STOP, 0u, 0u);
    const volatile uint32_t *ex = z32 + ZC_EXITED / 4;
    /* a queued server sees the stop request as soon as it runs; past
     * SRV_STOP_DEADLINE_S (the GPU busy with other work for that long, or
     * hung) the batch call fails instead of spinning on */
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1; *ex != g.srv_id; ++spin) {
        if ((spin & 4095u) == 0u) {
            const hipError_t e = hipStreamQuery(g.sstream);
            if (e == hipSuccess && *ex != g.srv_id) {
                g.srv_on = false;
                return fail("single-call server ended without its exit word");
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(SRV_STOP_DEADLINE_S))
                return fail("single-call server did not leave within %d s of a stop request", SRV_STOP_DEADLINE_S);
            if (e != hipSuccess && e != hipErrorNotReady) {
                g.srv_on = false;
                return fail("HIP error %d (%s) in the single-call server", (int)e, hipGetErrorString(e));
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    g.srv_on = false;
    return true;
}

EXPORT bool poporon_encode(poporon_t *h, uint8_t *data, size_t size, uint8_t *parity)
{
    if (!h || !data || !parity)
        return false;
    if (h->fec_type == PPLN_FEC_BCH && size < h->bch.dbytes) /* src/encode.c:210-212 */
        return false;
    if (h->fec_type == PPLN_FEC_LDPC) { /* src/encode.c:147-197: the host batch of one */
        if (size != h->ldpc->info_bytes)
            return fail("LDPC encode size %zu != info bytes %u", size, (unsigned)h->ldpc->info_bytes);
        return poporon_ldpc_encode_batch(h, data, size, parity, h->ldpc->parity_bytes, 1);
    }
    if (h->fec_type != PPLN_FEC_RS && h->fec_type != PPLN_FEC_BCH)
        return false;
    if (size > 65535) /* the reference's uint16 counter loops forever here (quirk Q7) */
        return fail("size %zu > 65535", size);
    if (!gpu_init(h))
        return false;
    DeviceGuard dg(h->gpu.device);
    GpuCtx &g = h->gpu;
    const size_t nr = par_bytes(h);
    /* one RS codeword: rs_enc1_k reads the message from and writes the parity
     * to coherent host memory and signals its completion word there (one
     * launch, no copies, no stream synchronisation) */
    /* (codes with fewer roots, h->nrsplit, the same way: their encq rows, P.nr) */
    if (h->fec_type == PPLN_FEC_RS && (h->fast || h->nrsplit) && size >= 1 && size <= kmax(h) && ensure_zc(g)) {
        memcpy(g.zc + ZC_DATA, data, size);
        const int sv = serve_enabled() && !g.timing ? srv_call(h, RS_SRV_ENCODE, (uint32_t)size, 0u) : -1;
        if (sv == 0)
            return false;
        if (sv < 0) {
            const uint32_t seq = zc_arm(g);
            KernelTimer t(g, POPORON_AMD_KERNEL_ENCODE, g.stream);
            HIP_OK(rsk_encode1_nr(g.tab, g.zc_dev + ZC_DATA, g.zc_dev + ZC_PAR, (uint32_t)size, (uint32_t)nr,
                                  reinterpret_cast<uint32_t *>(g.zc_dev + ZC_FLAG), seq, g.stream));
            t.done();
            if (!zc_wait(g, seq))
                return false;
        }
        memcpy(parity, g.zc + ZC_PAR, nr);
        return true;
    }
    /* general parameters: rsgw_encode_k on coherent host memory, the same way */
    if (h->fec_type == PPLN_FEC_RS && h->generic && gen_wave(h, 1, true, size) && ensure_zc(g)) {
        memcpy(g.zc + GZ_DATA, data, size);
        const int sv = serve_enabled() && !g.timing ? srv_call(h, RS_SRV_ENCODE, (uint32_t)size, 0u) : -1;
        if (sv == 0)
            return false;
        if (sv < 0) {
            RsGenParams prm = h->gen;
            prm.size = (uint32_t)size;
            const uint32_t seq = zc_arm(g);
            KernelTimer t(g, POPORON_AMD_KERNEL_ENCODE, g.stream);
            HIP_OK(rsgw_encode(g.gtab, &prm, g.zc_dev + GZ_DATA, size, g.zc_dev + GZ_PAR, nr, 1,
                               reinterpret_cast<uint32_t *>(g.zc_dev + ZC_FLAG), seq, g.num_cu, g.stream));
            t.done();
            if (!zc_wait(g, seq))
                return false;
        }
        memcpy(parity, g.zc + GZ_PAR, nr);
        return true;
    }
    const size_t off_p = (size + 15) & ~(size_t)15;
    if (!ensure_stage(h, off_p + nr + 16))
        return false;
    /* pinned mirror: one H2D copy in, one D2H copy out */
    if (size) {
        memcpy(g.hstage, data, size);
        HIP_OK(hipMemcpyAsync(g.stage, g.hstage, size, hipMemcpyHostToDevice, g.stream));
    }
    if (!launch_encode(h, g.stage, size, g.stage + off_p, nr, size, 1, g.stream))
        return false;
    HIP_OK(hipMemcpyAsync(g.hstage + off_p, g.stage + off_p, nr, hipMemcpyDeviceToHost, g.stream));
    HIP_OK(hipStreamSynchronize(g.stream));
    memcpy(parity, g.hstage + off_p, nr);
    return true;
}

/* src/decode.c:542-590: data bytes and corrected_num are written on success only */
static bool bch_decode_one(poporon_t *h, uint8_t *data, size_t size, uint8_t *parity, size_t *corrected_num)
{
    if (size < h->bch.dbytes)
        return false;
    if (!gpu_init(h))
        return false;
    DeviceGuard dg(h->gpu.device);
    GpuCtx &g = h->gpu;
    const size_t db = h->bch.dbytes, pb = h->bch.pbytes;
    if (!ensure_stage(h, db + pb + 2 + 16))
        return false;
    uint8_t *dd = g.stage, *dp = g.stage + db, *dok = dp + pb;
    if (db)
        HIP_OK(hipMemcpyAsync(dd, data, db, hipMemcpyHostToDevice, g.stream));
    if (pb)
        HIP_OK(hipMemcpyAsync(dp, parity, pb, hipMemcpyHostToDevice, g.stream));
    if (!launch_decode(h, {.data = dd, .ds = db, .par = dp, .ps = pb, .size = db, .count = 1, .ok = dok,
                           .corrected = dok + 1, .s = g.stream}))
        return false;
    uint8_t res[2];
    uint8_t out[4];
    HIP_OK(hipMemcpyAsync(res, dok, 2, hipMemcpyDeviceToHost, g.stream));
    if (db)
        HIP_OK(hipMemcpyAsync(out, dd, db, hipMemcpyDeviceToHost, g.stream));
    HIP_OK(hipStreamSynchronize(g.stream));
    if (!res[0])
        return false;
    memcpy(data, out, db);
    if (corrected_num)
        *corrected_num = res[1];
    return true;
}

/* One RS codeword on the device: false only for a device-side failure (no
 * usable GPU, a HIP error); the decode outcome goes to *success / *fixed. */
static bool rs_decode_one(poporon_t *h, uint8_t *data, size_t size, uint8_t *parity, bool *success_out,
                          size_t *fixed_out)
{
    size_t fixed = 0;
    bool success = false;
    if (!gpu_init(h))
        return false;
    {
        DeviceGuard dg(h->gpu.device);
        GpuCtx &g = h->gpu;
        const size_t nr = h->rs->num_roots;
        if ((h->fast || h->nrsplit) && ensure_zc(g)) {
            /* rs_dec1_k: the whole decode of one codeword in one launch, reading
             * the codeword, the erasure slots or the external syndromes from
             * coherent host memory and writing back the corrected bytes, ok and
             * corrected_num, then its completion word */
            uint8_t *z = g.zc;
            memcpy(z + ZC_DATA, data, size);
            memcpy(z + ZC_PAR, parity, nr);
            uint32_t mode = 0;
            if (h->ext_syndrome) {
                mode = 2; /* values > 255 are refused by the kernel (out-of-table in the reference) */
                memcpy(z + ZC_EXT, h->ext_syndrome, nr * sizeof(uint16_t));
            } else if (h->erasure) {
                mode = 1;
                const poporon_erasure_t *e = h->erasure;
                /* the reference reads slots by root ordinal (quirks Q2/Q3): nr
                 * slots, those past the list's capacity read as 0; the count as
                 * it is (past num_roots: refused for a dirty codeword, Q5) */
                uint32_t *pos = reinterpret_cast<uint32_t *>(z + ZC_POS);
                const size_t have = std::min<size_t>(e->capacity, nr);
                memcpy(pos, e->erasure_positions, have * sizeof(uint32_t));
                memset(pos + have, 0, (nr - have) * sizeof(uint32_t));
                *reinterpret_cast<uint32_t *>(z + ZC_CNT) = e->erasure_count;
            }
            const RsCorrParams prm = corr_params(h, size);
            uint8_t *zd = g.zc_dev;
            const int sv = serve_enabled() && !g.timing && prm.pad == (int32_t)(RS_NN - nr - size)
                               ? srv_call(h, RS_SRV_DECODE, (uint32_t)size, mode)
                               : -1;
            if (sv == 0)
                return false;
            if (sv < 0) {
                const uint32_t seq = zc_arm(g);
                KernelTimer t(g, POPORON_AMD_KERNEL_SINGLE, g.stream);
                HIP_OK(rsk_decode1(g.tab, &prm, mode, zd + ZC_DATA, zd + ZC_PAR, nullptr,
                                   reinterpret_cast<const uint32_t *>(zd + ZC_POS), zd + ZC_CNT, 4u,
                                   reinterpret_cast<const uint16_t *>(zd + ZC_EXT), zd + ZC_OK, zd + ZC_COR,
                                   reinterpret_cast<uint32_t *>(zd + ZC_FLAG), seq, g.stream));
                t.done();
                if (!zc_wait(g, seq))
                    return false;
            }
            memcpy(data, z + ZC_DATA, size);
            memcpy(parity, z + ZC_PAR, nr);
            success = z[ZC_OK] != 0;
            fixed = z[ZC_COR];
        } else if (gen_wave(h, 1, false, size) && ensure_zc(g)) {
            /* general parameters, one wave (rsgw_decode_k): the row, the slots
             * or the external syndromes read from coherent host memory, the
             * corrected bytes, ok and corrected_num written back there, then
             * the completion word (no copies, no stream synchronisation) */
            const uint32_t nn = h->rs->gf->field_size;
            uint8_t *z = g.zc, *zd = g.zc_dev;
            memcpy(z + GZ_DATA, data, size);
            memcpy(z + GZ_PAR, parity, nr);
            const uint16_t *ext = nullptr;
            const uint32_t *pos32 = nullptr;
            const uint8_t *cnt = nullptr;
            bool refuse = false;
            if (h->ext_syndrome) {
                for (size_t i = 0; i < nr; i++)
                    refuse |= h->ext_syndrome[i] > nn; /* out-of-table index in the reference */
                memcpy(z + GZ_EXT, h->ext_syndrome, nr * sizeof(uint16_t));
                ext = reinterpret_cast<const uint16_t *>(zd + GZ_EXT);
            } else if (h->erasure) {
                const poporon_erasure_t *e = h->erasure;
                uint32_t *pos = reinterpret_cast<uint32_t *>(z + GZ_POS);
                const size_t have = std::min<size_t>(e->capacity, nr); /* stale slots read as the reference (Q2/Q3) */
                memcpy(pos, e->erasure_positions, have * sizeof(uint32_t));
                memset(pos + have, 0, (nr - have) * sizeof(uint32_t));
                z[GZ_CNT] = (uint8_t)std::min<uint32_t>(e->erasure_count, 255u); /* past nr: refused if dirty (Q5) */
                pos32 = reinterpret_cast<const uint32_t *>(zd + GZ_POS);
                cnt = zd + GZ_CNT;
            }
            if (refuse) {
                fail("external syndrome > field size: undefined in the reference, refused");
            } else {
                const int sv = serve_enabled() && !g.timing
                                   ? srv_call(h, RS_SRV_DECODE, (uint32_t)size, ext ? 2u : pos32 ? 1u : 0u)
                                   : -1;
                if (sv == 0)
                    return false;
                if (sv < 0) {
                    const RsGenParams prm = gen_params(h, size);
                    const uint32_t seq = zc_arm(g);
                    KernelTimer t(g, POPORON_AMD_KERNEL_CORRECT, g.stream);
                    HIP_OK(rsgw_decode(g.gtab, &prm, zd + GZ_DATA, size, zd + GZ_PAR, nr, 1, ext, nr, nullptr, pos32,
                                       nr, cnt, zd + GZ_OK, zd + GZ_COR, nullptr, nullptr,
                                       reinterpret_cast<uint32_t *>(zd + ZC_FLAG), seq, g.num_cu, g.stream));
                    t.done();
                    if (!zc_wait(g, seq))
                        return false;
                }
                memcpy(data, z + GZ_DATA, size);
                memcpy(parity, z + GZ_PAR, nr);
                success = z[GZ_OK] != 0;
                fixed = z[GZ_COR];
            }
        } else {
            /* general parameters (rs_generic.hip): everything through the pinned
             * mirror, one H2D copy of [data | parity | ok | cor | pad | syndromes
             * (nr x u16) or slots (nr x u32) + count], the kernel, one D2H copy of
             * [data | parity | ok | cor] */
            const size_t off_p = size, off_ok = size + nr, off_cor = off_ok + 1;
            const size_t off_x = (off_cor + 1 + 15) & ~(size_t)15;
            if (!ensure_stage(h, off_x + nr * 4 + 16))
                return false;
            uint8_t *hs = g.hstage;
            const uint16_t *ext = nullptr;
            const uint32_t *pos32 = nullptr;
            const uint8_t *pos8 = nullptr;
            const uint8_t *cnt = nullptr;
            bool refuse = false;
            size_t in_bytes = off_cor + 1;
            memcpy(hs, data, size);
            memcpy(hs + off_p, parity, nr);
            if (h->ext_syndrome) {
                for (size_t i = 0; i < nr; i++)
                    refuse |= h->ext_syndrome[i] > h->rs->gf->field_size; /* out-of-table index in the reference */
                memcpy(hs + off_x, h->ext_syndrome, nr * sizeof(uint16_t));
                in_bytes = off_x + nr * sizeof(uint16_t);
                ext = (const uint16_t *)(g.stage + off_x);
            } else if (h->erasure) {
                const poporon_erasure_t *e = h->erasure;
                memset(hs + off_x, 0, nr * 4);
                memcpy(hs + off_x, e->erasure_positions, std::min<size_t>(e->capacity, nr) * sizeof(uint32_t));
                /* counts past num_roots (quirk Q5) reach the kernel clamped to 255:
                 * refused there only for a dirty codeword */
                hs[off_x + nr * 4] = (uint8_t)std::min<uint32_t>(e->erasure_count, 255u);
                in_bytes = off_x + nr * 4 + 1;
                pos32 = (const uint32_t *)(g.stage + off_x);
                cnt = g.stage + off_x + nr * 4;
                /* a fewer-roots code whose nr slots (the count's and the stale
                 * ones the reference reads, Q2) all fit a byte below 255: u8
                 * slots, so the errata kernels take it (launch_decode) */
                const uint32_t *pv = reinterpret_cast<const uint32_t *>(hs + off_x);
                bool small = h->nrsplit;
                for (size_t i = 0; i < nr && small; i++)
                    small = pv[i] < 255u;
                if (small) {
                    uint8_t sl[RS_NR];
                    for (size_t i = 0; i < nr; i++)
                        sl[i] = (uint8_t)pv[i];
                    memset(hs + off_x, 0, nr * 4);
                    memcpy(hs + off_x, sl, nr); /* a row of nr u8 slots, 4-byte aligned, stride nr * 4 */
                    pos32 = nullptr;
                    pos8 = g.stage + off_x;
                }
            }
            if (refuse) {
                fail("external syndrome > field size: undefined in the reference, refused");
            } else {
                HIP_OK(hipMemcpyAsync(g.stage, hs, in_bytes, hipMemcpyHostToDevice, g.stream));
                if (!launch_decode(h, {.data = g.stage, .ds = size, .par = g.stage + off_p, .ps = nr, .size = size,
                                       .count = 1, .ext_syn = ext, .ext_stride = nr, .pos8 = pos8, .pos32 = pos32,
                                       .pos_stride = pos8 ? nr * 4 : nr, .cnt = cnt, .ok = g.stage + off_ok,
                                       .corrected = g.stage + off_cor, .s = g.stream}))
                    return false;
                HIP_OK(hipMemcpyAsync(hs, g.stage, off_cor + 1, hipMemcpyDeviceToHost, g.stream));
                HIP_OK(hipStreamSynchronize(g.stream));
                memcpy(data, hs, size);
                memcpy(parity, hs + off_p, nr);
                success = hs[off_ok] != 0;
                fixed = hs[off_cor];
            }
        }
    }
    *success_out = success;
    *fixed_out = fixed;
    return true;
}

EXPORT bool poporon_decode(poporon_t *h, uint8_t *data, size_t size, uint8_t *parity, size_t *corrected_num)
{
    if (!h || !data || !parity || !size)
        return false;
    if (h->fec_type == PPLN_FEC_BCH)
        return bch_decode_one(h, data, size, parity, corrected_num);
    if (h->fec_type == PPLN_FEC_LDPC) {
        /* src/decode.c:489-540: soft when the config asks for it and brought LLRs;
         * corrected_num is the iteration count, written on success only */
        if (size != h->ldpc->info_bytes)
            return fail("LDPC decode size %zu != info bytes %u", size, (unsigned)h->ldpc->info_bytes);
        const int8_t *llr = h->ldpc_soft ? h->ldpc_llr : nullptr;
        uint8_t ok = 0;
        uint32_t it = 0;
        if (!poporon_ldpc_decode_batch(h, data, size, parity, h->ldpc->parity_bytes, llr, h->ldpc->codeword_bits, 1,
                                       &ok, &it, nullptr, 0))
            return false;
        h->ldpc_last_iterations = it;
        if (!ok)
            return false;
        if (corrected_num)
            *corrected_num = it;
        return true;
    }
    if (h->fec_type != PPLN_FEC_RS)
        return false;
    size_t fixed = 0;
    bool success = false;
    if (check_decode_size(h, size) && !rs_decode_one(h, data, size, parity, &success, &fixed)) {
        /* no usable device / a HIP failure: not a decode outcome.  The
         * reference never reports more than num_roots corrections, so the
         * sentinel tells this apart from "uncorrectable" (false, count 0..32);
         * poporon_amd_last_error() says what failed */
        h->last_corrected = POPORON_AMD_DEVICE_ERROR;
        if (corrected_num)
            *corrected_num = POPORON_AMD_DEVICE_ERROR;
        return false;
    }
    h->last_corrected = fixed;
    if (corrected_num)
        *corrected_num = fixed;
    return success;
}
