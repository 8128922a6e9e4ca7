// workspace.cpp -- the plan workspaces' layouts (workspace.hpp).  Host only.
#include "workspace.hpp"

namespace psvi {

int64_t eps_stride(const psvi_plan& p) { return (p.Peps + 3) / 4 * 4; }

bool tiled_ok(const psvi_plan& p) {
    return p.family == PSVI_FAMILY_FULLCOV && p.fuse_sample && p.tiles_total > 0 &&
           3 * p.tiles_total * 4096 * (int64_t)sizeof(float) < 0x7fffffff - 16;
}
size_t tiled_floats(const psvi_plan& p) {
    return tiled_ok(p) ? 3 * (size_t)p.tiles_total * 4096 : 0;
}

namespace {

// Every layout below continues the carve of the one it embeds.

StepWs carve_step(const psvi_plan& p, WsCarve& c) {
    StepWs o{};
    if (p.family == PSVI_FAMILY_FULLCOV) {
        const size_t n = (size_t)p.d.S * p.rows_tot[p.rank];
        o.x = c.take<float>(n);
        o.g = c.take<float>(n + 64);
        if (o.g) o.g_pad = o.g + n;
    } else {
        o.acc = c.take<float>((size_t)p.acc_count);
    }
    o.bytes = c.bytes();
    return o;
}

OuterWs carve_outer(const psvi_plan& p, WsCarve& c) {
    const size_t S = p.d.S, M = p.d.M, D = plan_in_dim(p);
    OuterWs o{};
    o.step = carve_step(p, c);
    o.nll = c.take<float>(S * M);
    o.rowcoef = c.take<float>(2 * S);
    o.ck = c.take<float>(S);
    o.sck = c.take<float>(1);
    o.stats = c.take<double>(2 * S);
    o.du = c.take<float>(S * M * D);
    if (p.lik == PSVI_LIK_GAUSSIAN) o.dz = c.take<float>(S * M);
    o.bytes = c.bytes();
    return o;
}

}  // namespace

StepWs step_ws(const psvi_plan& p, void* base) {
    WsCarve c(base);
    return carve_step(p, c);
}

LoopWs loop_ws(const psvi_plan& p, void* base) {
    WsCarve c(base);
    LoopWs o{};
    o.step = carve_step(p, c);
    const size_t es = (size_t)eps_stride(p);
    for (int k = 0; k < 2; ++k) {
        o.ebuf[k] = c.take<float>(es + 64);
        if (o.ebuf[k]) o.pads[k] = o.ebuf[k] + p.Peps;
    }
    o.pads[2] = o.step.g_pad;
    if (tiled_ok(p)) o.tstate = c.take<float>(tiled_floats(p));
    if (p.bf_stream) {
        for (int k = 0; k < 2; ++k) o.pbuf[k] = c.take<uint16_t>(3 * (size_t)p.eps_planes.pl);
        o.pbuf_bytes = align256(3 * sizeof(uint16_t) * (size_t)p.eps_planes.pl);
    }
    o.bytes = c.bytes();
    return o;
}

OuterWs outer_ws(const psvi_plan& p, void* base) {
    WsCarve c(base);
    return carve_outer(p, c);
}

EvalWs eval_ws(const psvi_plan& p, void* base) {
    const size_t S = p.d.S, M = p.d.M, C = p.lay[p.L - 1].dout;
    WsCarve c(base);
    EvalWs o{};
    o.outer = carve_outer(p, c);
    o.out = c.take<float>(S * M * C);
    o.W = c.take<float>(S);
    o.bytes = c.bytes();
    return o;
}

HvpWs hvp_ws(const psvi_plan& p, void* base) {
    const size_t S = p.d.S, M = p.d.M, D = p.lay[0].din, nt = p.n_tot;
    WsCarve c(base);
    HvpWs o{};
    o.step = carve_step(p, c);
    o.xd = c.take<float>(S * nt);
    const size_t ns = rop_splits(p);  // the R-op's row-block slots (summed into slot 0)
    o.G = c.take<float>(ns * S * nt);
    o.Gd = c.take<float>(ns * S * nt);
    o.du = c.take<float>(S * M * D);
    o.nlld = c.take<float>(S * M);
    if (p.lik == PSVI_LIK_GAUSSIAN) o.dzd = c.take<float>(S * M);
    if (p.family == PSVI_FAMILY_FULLCOV)
        o.part2 = c.take<float>(std::max({(size_t)p.fwd.n() * S, (size_t)p.n_fp_slots * kKsPass,
                                          (size_t)p.n_fs_slots * kKsPass}) *
                                kFwdRows);  // item-grid or either segment table's slots
    o.bytes = c.bytes();
    return o;
}

}  // namespace psvi
