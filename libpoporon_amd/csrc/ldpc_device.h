/*
 * ldpc_device.h -- device view of an LDPC handle's graph and the launchers of
 * the LDPC kernels (ldpc.hip), built by api.cpp from ldpc_graph.h's tables.
 */
#ifndef POPORON_AMD_LDPC_DEVICE_H
#define POPORON_AMD_LDPC_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

struct LdpcDev {
    uint32_t info_bits, parity_bits, codeword_bits;
    uint32_t info_bytes, parity_bytes, codeword_bytes;
    uint32_t num_checks, num_bits, num_edges;
    /* device arrays (one allocation, owned by the handle) */
    const uint32_t *row_ptr, *col_idx, *col_ptr, *edge_idx;
    /* gather tables, NULL when that interleaver is off */
    const uint32_t *inner_forward, *inner_inverse, *outer_forward, *outer_inverse;
};

#define LDPC_LDS_MAX (160u * 1024u) /* one workgroup may hold the CU's whole LDS */

#ifdef __cplusplus
extern "C" {
#endif

/* dynamic LDS of the decode kernel with the messages in LDS, and the bytes of
 * one workgroup's slice of the global workspace otherwise */
size_t ldpck_decode_lds_bytes(const LdpcDev *prm);
size_t ldpck_slice_bytes(const LdpcDev *prm);
/* the dynamic LDS a decode workgroup can get: LDPC_LDS_MAX less the kernel's static LDS
 * (needs the device: call with the handle's device current) */
size_t ldpck_decode_lds_room(void);
/* workgroups of a decode launch (each takes rows blockIdx.x, + gridDim.x, ...) */
uint32_t ldpck_decode_grid(const LdpcDev *prm, size_t count, int num_cu, bool lds);

hipError_t ldpck_encode(const LdpcDev *prm, uint8_t *data, size_t dstride, uint8_t *parity, size_t pstride,
                        size_t count, int num_cu, hipStream_t stream);
hipError_t ldpck_check(const LdpcDev *prm, const uint8_t *data, size_t dstride, const uint8_t *parity, size_t pstride,
                       size_t count, uint8_t *dirty, int num_cu, hipStream_t stream);
/* lds: messages in LDS; else in ws, grid * ldpck_slice_bytes bytes */
hipError_t ldpck_decode(const LdpcDev *prm, uint8_t *data, size_t dstride, const uint8_t *parity, size_t pstride,
                        const int8_t *llr, size_t lstride, size_t count, uint8_t *ok, uint32_t *iterations,
                        uint8_t *hard, size_t hstride, uint32_t max_iterations, bool lds, uint8_t *ws, uint32_t grid,
                        hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif
