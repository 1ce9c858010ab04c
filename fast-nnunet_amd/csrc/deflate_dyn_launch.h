// deflate_dyn_launch.h - how the host code of fnn_deflate_labels_dyn (csrc/deflate.hip) launches the kernels of
// csrc/deflate_dyn.hip.  Host only.
#pragma once
#include "deflate_dyn_core.h"
#include <hip/hip_runtime.h>

// pass 0: deflate_dyn_count_kernel, pass 1: deflate_dyn_emit_kernel, one wave per chunk; `elem`: the bytes of an element
// in the file, `narrow`: every second byte of a 2-byte map.  hdr_bits[c]: the bits of chunk c's block and table header, 0
// where it took the fixed code; rec: DF_DYN_REC_DWORDS dwords per chunk (deflate_dyn_core.h).
struct DfDynArgs {
    const uint8_t *in;
    long long n_bytes, chunks;
    const uint32_t *x2k;
    uint16_t *seg_bits;
    unsigned *chunk_bytes;
    uint32_t *chunk_crc, *hdr_bits, *rec;
    const long long *off;
    uint8_t *out;
};
void df_dyn_launch(int pass, int elem, bool narrow, const DfDynArgs &a, hipStream_t st);
