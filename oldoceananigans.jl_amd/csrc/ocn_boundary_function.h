// ocn_boundary_function.h -- FluxBoundaryCondition(func, field_dependencies, parameters) evaluated on the device
// (BoundaryConditions/continuous_boundary_function.jl:104-154, Utils/user_function_arguments.jl:22-39).
//
// The host calls the user's function once with symbols and records the operations as a list of ocn_expr_ins_t in SSA form: instruction n
// defines value n, operands name earlier values. boundary_function_kernel evaluates such lists at every point of a boundary into the dense
// (Na, Nb) array of an ordinary array-valued Flux condition -- the epilogue kernels, the shell kernel and compute_flux_bcs then see an
// array and nothing else.
//
// One launch serves all functions of a model: blockIdx.z selects the function, one thread per boundary point, the first tangential
// direction across the lanes. The instruction words are the same for every thread of a block (scalar loads, no divergence inside a wave);
// the values of a thread are indexed at run time, so they live in LDS, slot-major: vals[slot][thread], 64 slots x 128 threads x 8 B = 64 KB,
// consecutive lanes in consecutive banks. A thread only ever touches its own column: no barrier. At most Nx Ny points per function: this is
// not a throughput kernel.
//
// Arithmetic: the translation unit is compiled with -ffp-contract=off; every instruction is ONE IEEE operation (sqrt and / are the
// correctly rounded ones), in the order the user's function performed them.
#pragma once
#include "ocn_device.h"
#include "ocn_open_boundary.h"   // jl_min, jl_max
#include <cmath>

#define BF_MAX_INS 64            // instructions of a program (OCN_EXPR_MAX_INSTRUCTIONS)
#define BF_MAX_DEPS 8            // field dependencies of a function (OCN_EXPR_MAX_DEPENDENCIES)
#define BF_MAX_FUNCTIONS 16      // functions of one model
#define BF_LANES 64
#define BF_ROWS 2
#define BF_THREADS (BF_LANES * BF_ROWS)

// a dependency read at the boundary point (a, b) (0-based along the two tangential directions): the corner of its interpolation stencil at
// (0, 0) with the boundary-normal index folded in, the strides of a and b, and the interpolated directions, innermost first
struct BfDep {
    int field;                // slot of BfFields::p
    int n;                    // interpolated directions (0..2)
    long off, sa, sb;
    long st[2];
};

struct BfFunction {
    int n, ndeps;             // instructions, dependencies
    int Na, Nb;               // points along the two tangential directions
    double *out;              // dense (Na, Nb), column-major
    const double *xa, *xb;    // node coordinates along a and b at the condition's location (device tables of the grid)
    BfDep dep[BF_MAX_DEPS];
    ocn_expr_ins_t ins[BF_MAX_INS];
};

// the haloed arrays the dependencies name: the model's fields of this moment (they swap between stages), or the caller's arrays
struct BfFields {
    const double *p[OCN_MAX_FIELDS > BF_MAX_DEPS ? OCN_MAX_FIELDS : BF_MAX_DEPS];
};

// ℑ of a dependency: 0.5 (f[low] + f[low + 1]) per tangential direction, nested with st[0] innermost (ocn_diagnostics.h: dg_leaf)
__device__ __forceinline__ double bf_dependency(const BfDep &d, const double *p, int a, int b) {
    const double *q = p + (d.off + d.sa * a + d.sb * b);
    if (d.n == 0) return q[0];
    const long s0 = d.st[0];
    if (d.n == 1) return 0.5 * (q[0] + q[s0]);
    const long s1 = d.st[1];
    return 0.5 * (0.5 * (q[0] + q[s0]) + 0.5 * (q[s1] + q[s1 + s0]));
}

__global__ void __launch_bounds__(BF_THREADS) boundary_function_kernel(const BfFunction *table, BfFields fields, double time) {
    __shared__ double vals[BF_MAX_INS][BF_THREADS];
    const BfFunction &fn = table[blockIdx.z];
    const int a = blockIdx.x * BF_LANES + threadIdx.x, b = blockIdx.y * BF_ROWS + threadIdx.y;
    if (a >= fn.Na || b >= fn.Nb) return;
    const int t = threadIdx.y * BF_LANES + threadIdx.x;
    const int n = fn.n;
    for (int q = 0; q < n; ++q) {
        const ocn_expr_ins_t ins = fn.ins[q];
        // operands: validated on the host to name earlier values (unused ones are 0)
        const double x = vals[ins.a][t], y = vals[ins.b][t];
        double r;
        switch (ins.op) {
        case OCN_EXPR_CONST: r = ins.imm; break;
        case OCN_EXPR_COORD: r = ins.a == 0 ? fn.xa[a] : fn.xb[b]; break;
        case OCN_EXPR_TIME: r = time; break;
        case OCN_EXPR_FIELD: r = bf_dependency(fn.dep[ins.a], fields.p[fn.dep[ins.a].field], a, b); break;
        case OCN_EXPR_ADD: r = x + y; break;
        case OCN_EXPR_SUB: r = x - y; break;
        case OCN_EXPR_MUL: r = x * y; break;
        case OCN_EXPR_DIV: r = x / y; break;
        case OCN_EXPR_NEG: r = -x; break;
        case OCN_EXPR_ABS: r = fabs(x); break;
        case OCN_EXPR_MIN: r = jl_min(x, y); break;
        case OCN_EXPR_MAX: r = jl_max(x, y); break;
        case OCN_EXPR_SQRT: r = sqrt(x); break;
        case OCN_EXPR_EXP: r = exp(x); break;
        case OCN_EXPR_LOG: r = log(x); break;
        case OCN_EXPR_SIN: r = sin(x); break;
        case OCN_EXPR_COS: r = cos(x); break;
        case OCN_EXPR_TANH: r = tanh(x); break;
        case OCN_EXPR_POW: r = pow(x, y); break;
        case OCN_EXPR_LT: r = x < y ? 1.0 : 0.0; break;
        case OCN_EXPR_LE: r = x <= y ? 1.0 : 0.0; break;
        case OCN_EXPR_GT: r = x > y ? 1.0 : 0.0; break;
        case OCN_EXPR_GE: r = x >= y ? 1.0 : 0.0; break;
        default: r = x != 0.0 ? y : vals[ins.c][t]; break;          // OCN_EXPR_SELECT
        }
        vals[q][t] = r;
    }
    fn.out[a + (long)fn.Na * b] = vals[n - 1][t];
}
