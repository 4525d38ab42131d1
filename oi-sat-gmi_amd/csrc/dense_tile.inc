// The tile constants of the dense solver.  Included first inside each dense_*.hip unit's anonymous namespace.
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NB = 128;          // diagonal block / tile edge
constexpr int BK = 32;           // K step
constexpr int LDSW = 36;         // padded LDS row stride in floats (144 B, 16-B aligned)
constexpr int SB = 64;           // edge of the small GEMM tiles (dense_gemm.hip) and of the leaf pairs' row pieces (dense_chol.hip)

// wave priority of a group's kernels (oisat_set_share; BatchArgs::prio): the GEMMs, the leaf pairs, the diagonal block
__device__ __forceinline__ void group_prio(int p) {        // p is wave-uniform (a kernel argument)
    if (p == 3) __builtin_amdgcn_s_setprio(3);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
}
