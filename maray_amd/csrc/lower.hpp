// lower.hpp — lowered program container (product code).
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

struct Tape {
    std::vector<double> consts;
    std::vector<uint64_t> row_ops;
    std::vector<uint64_t> pix_ops;
    maray_tape_info info;
    std::vector<double> param_ranges;    // lo, hi per declared parameter; empty: no op reads a parameter (a version-2 program)
    // REFINE section (include/maray_tape.h): empty when no guarded conjunction has a Step(Sin) factor that can be bounded
    std::vector<double> refine_consts;
    std::vector<uint64_t> refine_ops;
    uint32_t refine_slots = 0, refine_outs = 0;

    maray_program program() const {
        maray_program p;
        p.version = param_ranges.empty() ? MARAY_TAPE_VERSION : MARAY_TAPE_VERSION_PARAMS;
        p.n_params = (uint32_t)(param_ranges.size() / 2);
        p.param_ranges = param_ranges.empty() ? nullptr : param_ranges.data();
        p.n_consts = (uint32_t)consts.size();
        p.consts = consts.data();
        p.n_row_ops = (uint32_t)row_ops.size();
        p.row_ops = row_ops.data();
        p.n_row_slots = info.n_row_slots;
        p.n_yvals = info.n_yvals;
        p.n_pix_ops = (uint32_t)pix_ops.size();
        p.pix_ops = pix_ops.data();
        p.n_pix_slots = info.n_pix_slots;
        p.n_app = info.n_app;
        return p;
    }
    maray_refine refine() const {
        maray_refine r;
        r.n_consts = (uint32_t)refine_consts.size();
        r.consts = refine_consts.data();
        r.n_ops = (uint32_t)refine_ops.size();
        r.ops = refine_ops.data();
        r.n_slots = refine_slots;
        r.n_outs = refine_outs;
        return r;
    }
};

void lower_scene(const Scene &scene, const maray_lower_opts &opts, Tape &out);   // throws Error

// Validate a program handed in through the tape-level ABI (bounds of every
// slot / constant / y-value / output reference); throws Error.
void validate_program(const maray_program &p);
// A program as the library holds it, from one handed in through the ABI: a version-2 struct ends at n_app and is not read
// past it (n_params = 0).  Throws Error on a null pointer.
maray_program load_program(const maray_program *p);
void validate_refine(const maray_program &p, const maray_refine &r);      // a REFINE section beside its program; throws Error
// Is v a value parameter p of the program may take?  (Inside its declared range, zeros compared by sign as well: a range
// that starts at +0.0 excludes -0.0, whose sign the lowering's "sign bit clear" statements would not survive.)
bool param_value_ok(const double *ranges, uint32_t p, double v);

}   // namespace maray
