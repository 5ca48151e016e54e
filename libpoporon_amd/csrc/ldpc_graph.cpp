/*
 * ldpc_graph.cpp -- see ldpc_graph.h.  Every table equals the reference's
 * for the same 10 parameters (tests/test_ldpc_cpu.py compares them with the
 * arrays recorded from the reference's own handle).
 */
#include "ldpc_graph.h"

namespace {

/* xoshiro128++ seeded through splitmix32 from one 32-bit seed, drawing 32-bit
 * words: the stream poporon_rng_create(XOSHIRO128PP, &seed, 4) /
 * poporon_rng_next(rng, &word, 4) gives (src/rng.c, rng.hip; pinned by
 * tests/golden/rng_golden.npz through the graph fixtures) */
struct Xoshiro {
    uint32_t s[4];
    static uint32_t mix(uint32_t z)
    {
        z = (z ^ (z >> 16)) * 0x85EBCA6Bu;
        z = (z ^ (z >> 13)) * 0xC2B2AE35u;
        return z ^ (z >> 16);
    }
    static uint32_t rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
    explicit Xoshiro(uint32_t seed)
    {
        s[0] = mix(seed + 0x6C078965u);
        s[1] = mix(s[0] + 0x9D2C5680u);
        s[2] = mix(s[1] + 0xEFC60000u);
        s[3] = mix(s[2] + 0x12345678u);
    }
    uint32_t next()
    {
        const uint32_t r = rotl(s[0] + s[3], 7) + s[0];
        const uint32_t t = s[1] << 9;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 11);
        return r;
    }
};

/* Fisher-Yates from the top, one word per step (src/ldpc.c:203-209, :267-273) */
void shuffle(std::vector<uint32_t> &v, uint32_t seed)
{
    Xoshiro rng(seed);
    for (size_t i = v.size(); i-- > 1;) {
        const size_t j = rng.next() % (i + 1);
        const uint32_t t = v[i];
        v[i] = v[j];
        v[j] = t;
    }
}

/* H = [A | D]: A holds `weight` draws per info bit (RANDOM: a row; QC_RANDOM:
 * a base row and a cyclic shift inside the lifting block), D is the dual
 * diagonal.  Two passes over the same random stream, as the reference does:
 * row sizes, then the columns in draw order; the diagonal's two entries close
 * each row.  Duplicate (row, column) draws stay duplicate edges. */
void build_matrix(LdpcGraph &g, bool qc, uint32_t weight, uint32_t lifting, uint32_t seed)
{
    const uint32_t P = g.parity_bits, K = g.info_bits;
    uint32_t base_rows = 0;
    if (qc) {
        if (lifting == 0) { /* automatic: parity_bits / 8 in [4, 256], rounded down to a power of two */
            lifting = P / 8;
            if (lifting < 4)
                lifting = 4;
            if (lifting > 256)
                lifting = 256;
            while (lifting & (lifting - 1))
                lifting &= lifting - 1;
        }
        base_rows = (uint32_t)(((uint64_t)P + lifting - 1) / lifting);
    }
    /* the row of one draw, or P and above for a QC edge that is dropped */
    auto draw = [&](Xoshiro &rng, uint32_t bit) -> uint32_t {
        if (!qc)
            return rng.next() % P;
        const uint32_t block_row = rng.next() % base_rows;
        const uint32_t shift = rng.next() % lifting;
        const uint32_t in_block = (bit % lifting + shift) % lifting;
        return block_row * lifting + in_block; /* uint32 arithmetic, as the reference */
    };

    std::vector<uint32_t> fill(P, 0);
    {
        Xoshiro rng(seed);
        for (uint32_t i = 0; i < K; i++)
            for (uint32_t j = 0; j < weight; j++) {
                const uint32_t r = draw(rng, i);
                if (r < P)
                    fill[r]++;
            }
    }
    g.row_ptr.assign((size_t)P + 1, 0);
    for (uint32_t r = 0; r < P; r++)
        g.row_ptr[r + 1] = g.row_ptr[r] + fill[r] + (r == 0 ? 1u : 2u);
    g.num_edges = g.row_ptr[P];
    g.col_idx.assign(g.num_edges, 0);
    fill.assign(P, 0);
    {
        Xoshiro rng(seed);
        for (uint32_t i = 0; i < K; i++)
            for (uint32_t j = 0; j < weight; j++) {
                const uint32_t r = draw(rng, i);
                if (r < P)
                    g.col_idx[g.row_ptr[r] + fill[r]++] = i;
            }
    }
    for (uint32_t r = 0; r < P; r++) {
        if (r > 0)
            g.col_idx[g.row_ptr[r] + fill[r]++] = K + r - 1;
        g.col_idx[g.row_ptr[r] + fill[r]++] = K + r;
    }

    /* column view: bit i's edges in row order (src/ldpc.c:386-406) */
    const uint32_t N = g.num_bits;
    g.col_ptr.assign((size_t)N + 1, 0);
    for (uint32_t e = 0; e < g.num_edges; e++)
        g.col_ptr[g.col_idx[e] + 1]++;
    for (uint32_t i = 0; i < N; i++)
        g.col_ptr[i + 1] += g.col_ptr[i];
    g.edge_idx.assign(g.num_edges, 0);
    std::vector<uint32_t> at(g.col_ptr.begin(), g.col_ptr.end() - 1);
    for (uint32_t e = 0; e < g.num_edges; e++)
        g.edge_idx[at[g.col_idx[e]]++] = e;
}

/* Block interleaver of `depth` rows with shuffled columns (src/ldpc.c:150-234):
 * bit i at (row, col) = (i / width, i % width) goes to perm[col] * depth + row;
 * targets past the codeword stay where they are. */
void build_inner(LdpcGraph &g, uint32_t depth, uint64_t seed)
{
    const uint32_t N = g.codeword_bits;
    if (depth == 0) {
        depth = N / 4;
        if (depth < 8)
            depth = 8;
        if (depth > 256)
            depth = 256;
    }
    const uint32_t width = (uint32_t)(((uint64_t)N + depth - 1) / depth);
    std::vector<uint32_t> perm(width);
    for (uint32_t i = 0; i < width; i++)
        perm[i] = i;
    shuffle(perm, (uint32_t)(seed ^ (uint64_t)N));
    g.inner_forward.resize(N);
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t row = i / width, col = i % width;
        uint64_t pos = i;
        if (row < depth) {
            pos = (uint64_t)(uint32_t)(perm[col] * depth) + row; /* the product wraps at 32 bits, the sum does not */
            if (pos >= N)
                pos = i;
        }
        g.inner_forward[i] = (uint32_t)pos;
    }
    std::vector<uint8_t> hit(N, 0);
    g.inner_bijective = true;
    g.inner_inverse.assign(N, 0);
    for (uint32_t i = 0; i < N; i++) {
        if (hit[g.inner_forward[i]]++)
            g.inner_bijective = false;
        g.inner_inverse[g.inner_forward[i]] = i;
    }
}

void build_outer(LdpcGraph &g, uint64_t seed)
{
    const uint32_t n = g.info_bytes;
    g.outer_forward.resize(n);
    for (uint32_t i = 0; i < n; i++)
        g.outer_forward[i] = i;
    shuffle(g.outer_forward, (uint32_t)(seed ^ (uint64_t)((size_t)g.info_bits ^ 0xDEADBEEF)));
    g.outer_inverse.assign(n, 0);
    for (uint32_t i = 0; i < n; i++)
        g.outer_inverse[g.outer_forward[i]] = i;
}

} // namespace

bool ldpc_graph_build(LdpcGraph &g, size_t block_size, uint32_t rate, uint32_t matrix_type, uint32_t column_weight,
                      bool use_outer_interleave, bool use_inner_interleave, uint32_t interleave_depth,
                      uint32_t lifting_factor, uint64_t seed)
{
    static const uint32_t info_num[6] = {1, 1, 2, 3, 4, 5}, parity_num[6] = {2, 1, 1, 1, 1, 1};
    if (block_size < 32 || block_size > 8192 || block_size % 4 != 0 || rate > 5)
        return false;
    g = LdpcGraph();
    g.info_bytes = (uint32_t)block_size;
    g.info_bits = g.info_bytes * 8;
    g.parity_bits = g.info_bits * parity_num[rate] / info_num[rate];
    g.codeword_bits = g.info_bits + g.parity_bits;
    g.parity_bytes = (g.parity_bits + 7) / 8;
    g.codeword_bytes = g.info_bytes + g.parity_bytes;
    g.num_checks = g.parity_bits;
    g.num_bits = g.codeword_bits;
    const uint32_t weight = column_weight < 3 ? 3 : column_weight > 8 ? 8 : column_weight;
    build_matrix(g, matrix_type == 2 /* PPRN_LDPC_QC_RANDOM */, weight, lifting_factor, (uint32_t)seed);
    g.inner = use_inner_interleave;
    g.outer = use_outer_interleave;
    if (g.inner)
        build_inner(g, interleave_depth, seed);
    if (g.outer)
        build_outer(g, seed);
    return true;
}
