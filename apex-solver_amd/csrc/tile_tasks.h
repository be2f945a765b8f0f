// tile_tasks.h -- the task records of the tile Cholesky / triangular-solve / PCG / selected-inversion kernels: plain structs
// that the host builds into lists (TilePlan, SelectedInverse) and the kernels read (chol_kernels.hip, sinv_kernels.hip).  No HIP
// type: host-only code (factor_schedule.cpp, sinv_lists.cpp) includes this file alone.
#pragma once

namespace apex {

constexpr int kNB = 144;   // S tile edge: 16*9 = 24*6, multiple of the 16-wide f64 MFMA

struct GemmTask {  // C = beta*C + alpha * A * B^T on 144x144 row-major tiles
    double* C;
    const double* A;
    const double* B;
};

struct PotrfTask {  // one diagonal tile: factor in place, inverse of the factor to Linv
    double* A;
    double* Linv;
    int K;
};

constexpr int kFlowFirstWriter = 16;   // FactorUnit::kind bit: the unit is the FIRST writer of a fill tile (nothing is read from the target)
constexpr int kFlowUnitsPerTile = 9;   // units per panel solve / update; the weight of a potrf in the version counters
struct FactorUnit {   // one workgroup of the dataflow factorisation of the top of the elimination tree (k_factor_flow)
    double* C;            // potrf: the diagonal tile (factorised in place); product: the target tile
    const double* A;      // potrf: L^-1 of the tile (written); product: left operand tile (panel solve: == C, in place)
    const double* B;      // product: right operand tile (panel solve: L^-1 of the column's diagonal tile)
    int wait_flag[3];     // indices into the version array, -1 = none: [0] the target's previous writer, [1] A final, [2] B final
    int wait_val[3];      // ... proceed when ver[flag] >= val
    int pub;              // index into the version array: += 1 per finished unit (kFlowUnitsPerTile per tile and writer), += 9 by a potrf
    int kind;             // 0 potrf + inverse, 1 panel solve C = A B^T (in place), 2 update C -= A B^T (one 48 x 48 block), 3 update, the whole tile (publishes 9)
    int strip;            // panel solve: 16-row strip 0..8 of C; update: 48 x 48 block 3 bi + bj of C; potrf: tile column (for the failure flag)
    int pad;
};

struct TriTask {   // one workgroup of a triangular-solve step (k_tri_step)
    const double* Mdiag;  // Linv of the step's diagonal tile
    const double* Moff;   // the off-diagonal tile this workgroup applies (unused when other < 0)
    int k;                // block solved in this step
    int other;            // block updated by this workgroup; -1: store the solved block instead
};

struct FlowTask {     // one workgroup of a dataflow triangular sweep (k_tri_fwd_flow / k_tri_bwd_flow)
    const double* mat;    // product task: the off-diagonal tile; solve task: L^-1 of the diagonal tile
    int src;              // product: the block whose solution the tile multiplies; solve: -1; fold only (distributed
                          // forward, a shared top block: right-hand side minus this rank's products, no solve): -2
    int dst;              // product: the block the product belongs to; solve: the block solved
    int part;             // product: its slot in the partial array; solve: first slot of the block's products
    int count;            // solve: number of products to wait for and fold
    // solve task, round 5 (single-GPU plans): the product of the block's LAST-ARRIVING source -- the link of the dependency chain --
    // is formed by the solve task itself (tile mat2 times the solution of block src2, into slot `slot2` of the fold, same
    // arithmetic, same place in the sum): one flag hop and one trip of the product through memory less per level.  src2 < 0: none
    const double* mat2 = nullptr;
    int src2 = -1;
    int slot2 = -1;
};

struct SymEntry {  // one tile of block-row I of the symmetric tile matrix
    int slot;      // tile slot
    int other;     // the other block index (column block for kind 0/2, row block for kind 1)
    int kind;      // 0: tile (I,other) other<I ; 1: tile (other,I) other>I (use transpose) ; 2: diagonal
};

struct SymTile { int slot, I, J; };  // a structurally non-zero tile (I >= J) of S

// ---- selected inversion (tile_sinv.h; the lists by name: sinv_lists.h) ----
constexpr int kSinvTransA = 1, kSinvTransB = 2, kSinvNeg = 4;   // SinvProd::op bits
struct SinvProd {   // one term op(A) op(B) of a sum (kSinvNeg: subtracted); A, B are 144 x 144 row-major tiles
    const double* A;
    const double* B;
    int op;
    int pad;
};
struct SinvTask {   // C := sum of the products [first, first + count), summed in list order (C is not read)
    double* C;
    int first;
    int count;
};

}  // namespace apex
