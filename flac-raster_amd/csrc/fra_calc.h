// fra_calc.h -- the validator of a band-math program (include/flac_raster_amd.h: the list under "A program is valid
// when").  k_calc (fra_calc.hip) interprets a caller's program: which stack slot a word reads, which band it loads and
// which output it stores all come from the program's words, so the host proves every one of them in range here, by
// simulating the stack, before anything is launched.  Plain C++: the library, the stand-alone check program and
// fra_calc_check (no context, no GPU) share it.  flac_raster/calc.py: validate is its Python twin, refusal by refusal.
#pragma once
#include <cstdint>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"

namespace fra_calcp {

// values a word pops and pushes; -1 for an unknown op
inline int pops_of(int op) {
  switch (op) {
    case FRA_CALC_CONST: case FRA_CALC_BAND: return 0;
    case FRA_CALC_STORE: case FRA_CALC_NEG: case FRA_CALC_ABS: case FRA_CALC_SQRT: case FRA_CALC_FLOOR:
    case FRA_CALC_NOT: return 1;
    case FRA_CALC_SELECT: return 3;
  }
  return op >= FRA_CALC_ADD && op <= FRA_CALC_OR ? 2 : -1;
}
inline int pushes_of(int op) { return op == FRA_CALC_STORE ? 0 : 1; }

// FRA_OK for a valid program over `channels` bands; *max_depth (may be null): the deepest the stack gets
inline int check_program(const fra_calc_program* p, int32_t channels, int* max_depth) {
  if (!p) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (p->ncode < 1 || p->ncode > FRA_CALC_MAX_CODE)
    return fra_internal_set_error(FRA_E_INVALID, "program of %d words outside 1 ... %d", p->ncode, FRA_CALC_MAX_CODE);
  if (p->nconst < 0 || p->nconst > FRA_CALC_MAX_CONST)
    return fra_internal_set_error(FRA_E_INVALID, "%d constants outside 0 ... %d", p->nconst, FRA_CALC_MAX_CONST);
  if (p->nout < 1 || p->nout > FRA_CALC_MAX_OUT)
    return fra_internal_set_error(FRA_E_INVALID, "%d outputs outside 1 ... %d", p->nout, FRA_CALC_MAX_OUT);
  if (p->flags & ~FRA_CALC_NODATA)
    return fra_internal_set_error(FRA_E_INVALID, "unknown band-math flags 0x%x", (unsigned)p->flags);
  if (channels < 1 || channels > 255)
    return fra_internal_set_error(FRA_E_INVALID, "%d source bands outside 1 ... 255", channels);
  int depth = 0, deepest = 0;
  unsigned stored = 0;
  for (int i = 0; i < p->ncode; i++) {
    const int op = p->code[i] & 0xff, arg = p->code[i] >> 8;
    const int pops = pops_of(op);
    if (pops < 0) return fra_internal_set_error(FRA_E_INVALID, "word %d: unknown op %d", i, op);
    if (op == FRA_CALC_BAND) {
      if (arg >= channels)
        return fra_internal_set_error(FRA_E_INVALID, "word %d: band %d of %d", i, arg, channels);
    } else if (op == FRA_CALC_CONST) {
      if (arg >= p->nconst)
        return fra_internal_set_error(FRA_E_INVALID, "word %d: constant %d of %d", i, arg, p->nconst);
    } else if (op == FRA_CALC_STORE) {
      if (arg >= p->nout) return fra_internal_set_error(FRA_E_INVALID, "word %d: output %d of %d", i, arg, p->nout);
      if (stored >> arg & 1) return fra_internal_set_error(FRA_E_INVALID, "word %d: output %d stored twice", i, arg);
      stored |= 1u << arg;
    } else if (arg != 0) {
      return fra_internal_set_error(FRA_E_INVALID, "word %d: op %d takes no argument (%d)", i, op, arg);
    }
    if (depth < pops) return fra_internal_set_error(FRA_E_INVALID, "word %d: stack underflow", i);
    depth += pushes_of(op) - pops;
    if (depth > FRA_CALC_MAX_DEPTH)
      return fra_internal_set_error(FRA_E_INVALID, "word %d: stack deeper than %d", i, FRA_CALC_MAX_DEPTH);
    if (depth > deepest) deepest = depth;
  }
  if (depth != 0)
    return fra_internal_set_error(FRA_E_INVALID, "word %d: %d values left on the stack at the end", p->ncode - 1, depth);
  for (int k = 0; k < p->nout; k++)
    if (!(stored >> k & 1))
      return fra_internal_set_error(FRA_E_INVALID, "word %d: output %d is never stored", p->ncode - 1, k);
  if (max_depth) *max_depth = deepest;
  return FRA_OK;
}

}  // namespace fra_calcp
