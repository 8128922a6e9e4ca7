// workspace.hpp -- the layout of every caller-allocated plan workspace: the
// single statement of its regions, their order and their sizes.  Each layout
// function serves the psvi_plan_query key (base nullptr: sizes only, every
// region nullptr) and the entry point's pointers.  Host only: no HIP call.
#pragma once
#include "psvi_internal.hpp"

namespace psvi {

// Philox offset between two steps' draws of a loop
int64_t eps_stride(const psvi_plan& p);
// tiled corr/m/v state: full-cov, world 1, one LDS pass of samples.  The
// write-through (sc1) stores of the stream kernel and the chunked kernel's
// tiled epilogue address all three arrays through ONE buffer descriptor
// (num_records 0x7fffffff, m / v at 32-bit byte offsets), so the whole state
// must stay below 2^31 bytes; larger plans keep corr / m / v packed (the
// chunked kernel with plain stores) instead of overflowing those offsets.
bool tiled_ok(const psvi_plan& p);
size_t tiled_floats(const psvi_plan& p);

// PSVI_Q_WS_BYTES (psvi_inner_step, psvi_elbo_grad), and the head of every
// other plan workspace.  Full-cov: the rank's x and g shards [S][rows], g
// followed by 64 floats (g_pad).  Otherwise acc [2 n_tot].
struct StepWs {
    float *x, *g, *g_pad;
    float* acc;
    size_t bytes;
};
StepWs step_ws(const psvi_plan& p, void* base);

// PSVI_Q_LOOP_WS_BYTES (psvi_inner_loop): the step workspace, two eps buffers
// [eps_stride] each followed by 64 floats, the tiled state (tiled_ok plans),
// two buffers of one draw's three bf16 planes (bf_stream plans).  pads: the 64
// floats behind each eps buffer and behind g (full-cov) -- zeroed with the
// tiled conversion; the streaming update's loads past a layer's last column
// block land there, unclamped.
struct LoopWs {
    StepWs step;
    float* ebuf[2];
    float* tstate;
    uint16_t* pbuf[2];
    size_t pbuf_bytes;  // of one plane buffer
    float* pads[3];
    size_t bytes;
};
LoopWs loop_ws(const psvi_plan& p, void* base);

// PSVI_Q_OUTER_WS_BYTES (psvi_outer_elbo_grad): the step workspace, the
// per-row NLL [S][M], row coefficients [S][2], ck [S], sum ck, per-sample
// stats [S][2] doubles, the per-sample input gradients [S][M][D]
struct OuterWs {
    StepWs step;
    float *nll, *rowcoef, *ck, *sck, *du;
    double* stats;
    float* dz;  // Gaussian plans: per-sample target gradients [S][M]
    size_t bytes;
};
OuterWs outer_ws(const psvi_plan& p, void* base);

// PSVI_Q_EVAL_WS_BYTES (psvi_evaluate, psvi_evaluate_regression): the outer
// workspace, the data rows' softmax [S][M][C] (bounded by M rows; a Gaussian
// plan's outputs [S][M]: C = 1) and the sample weights [S]
struct EvalWs {
    OuterWs outer;
    float *out, *W;
    size_t bytes;
};
EvalWs eval_ws(const psvi_plan& p, void* base);

// PSVI_Q_HVP_WS_BYTES (psvi_hvp) of the plans the R-op kernel runs (LeNet:
// lenet_tan_ws): the step workspace (x), x_dot [S][n_tot], G and G_dot
// [splits][S][n_tot], d_u parts [S][M][D], NLL_dot [S][M]
struct HvpWs {
    StepWs step;
    float *xd, *G, *Gd, *du, *nlld;
    float* dzd;    // Gaussian plans: per-sample target products [S][M]
    float* part2;  // full-cov: split-K slots of the tangent sample (pair launch)
    size_t bytes;
};
HvpWs hvp_ws(const psvi_plan& p, void* base);

}  // namespace psvi
