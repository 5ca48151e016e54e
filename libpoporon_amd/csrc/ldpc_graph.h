/*
 * ldpc_graph.h -- host construction of an LDPC code: sizes, the parity-check
 * matrix (CSR rows and the column view), the inner bit interleaver and the
 * outer byte interleaver, as the reference builds them (src/ldpc.c:150-601,
 * :814-872).  Plain C++: nothing here needs HIP, so handle creation runs on a
 * machine without a GPU and the file links into a stand-alone program.
 */
#ifndef POPORON_AMD_LDPC_GRAPH_H
#define POPORON_AMD_LDPC_GRAPH_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

struct LdpcGraph {
    uint32_t info_bits = 0, parity_bits = 0, codeword_bits = 0;
    uint32_t info_bytes = 0, parity_bytes = 0, codeword_bytes = 0;
    uint32_t num_checks = 0, num_bits = 0;
    /* edges actually placed (row_ptr[num_checks]); the QC builder drops the
     * edges whose row falls past parity_bits, so this can be below the
     * info_bits * weight + 2 * parity_bits - 1 the reference sizes its arrays by */
    uint32_t num_edges = 0;
    std::vector<uint32_t> row_ptr, col_idx;  /* CSR rows of H */
    std::vector<uint32_t> col_ptr, edge_idx; /* column view: the edges of bit i, in row order */
    bool inner = false, outer = false;
    /* inner bit interleaver (codeword_bits entries) and outer byte interleaver
     * (info_bytes entries); empty when off.  forward scatters: out[forward[i]] = in[i] */
    std::vector<uint32_t> inner_forward, inner_inverse;
    std::vector<uint32_t> outer_forward, outer_inverse;
    /* false when inner_forward is not a permutation (depth * width !=
     * codeword_bits): the reference's inverse table then keeps uninitialised
     * words and its decode reads them, so such a code is not served */
    bool inner_bijective = true;
};

/* false for parameters poporon_ldpc_create refuses (src/ldpc.c:821-827) */
bool ldpc_graph_build(LdpcGraph &g, size_t block_size, uint32_t rate, uint32_t matrix_type, uint32_t column_weight,
                      bool use_outer_interleave, bool use_inner_interleave, uint32_t interleave_depth,
                      uint32_t lifting_factor, uint64_t seed);

#endif
