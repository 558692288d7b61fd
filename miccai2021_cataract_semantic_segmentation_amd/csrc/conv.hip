// catseg_conv2d_fwd / _bwd_data / _bwd_weight(_workspace): the one entry point per direction of the implicit-GEMM convolutions.  No kernel lives
// here: a call is checked for what the operand forms share (the table in catseg.h) and handed to its arithmetic's file, which keeps the form's
// own checks and messages.  Whatever refuses, the message starts with the entry point's name.
#include <string.h>
#include "slabs.h"

namespace {

bool is_f16x2(int form) { return form == CATSEG_OPERANDS_F16X2 || form == CATSEG_OPERANDS_F16X2_BLOCKED; }
bool is_bf16x3(int form) { return form == CATSEG_OPERANDS_BF16X3 || form == CATSEG_OPERANDS_BF16X3_BLOCKED; }

int named(const char* fn, int rc) {
  if (rc != CATSEG_OK) {
    char msg[400];
    strncpy(msg, catseg_last_error(), sizeof msg - 1);
    msg[sizeof msg - 1] = 0;
    catseg_set_error("%s: %s", fn, msg);
  }
  return rc;
}

int check_operands(int form, const void* scale_a, const void* scale_b) {
  CS_REQUIRE(form >= CATSEG_OPERANDS_F32 && form <= CATSEG_OPERANDS_F16X2_BLOCKED, "unknown operand form %d", form);
  CS_REQUIRE(is_f16x2(form) || (scale_a == nullptr && scale_b == nullptr), "a scale record goes with f16x2 operands only");
  return CATSEG_OK;
}

int fwd(const catseg_conv_fwd_desc* q, hipStream_t st) {
  CS_REQUIRE(q != nullptr, "null descriptor");
  if (int e = check_operands(q->operands, q->x_scale, q->w_scale)) return e;
  CS_REQUIRE(q->operands != CATSEG_OPERANDS_F16X2, "planar f16x2 operands are for backward-weight only");
  if (q->residual || q->relu) {
    CS_REQUIRE(q->operands != CATSEG_OPERANDS_BF16X3, "residual / relu need fp32 or blocked operands, not planar bf16x3");
    CS_REQUIRE(q->zero_to == 0 && q->bn_part == nullptr, "residual / relu exclude zero_to and bn_part");
  }
  return q->operands == CATSEG_OPERANDS_F32 ? cs_conv_fwd_f32(q, st) : is_bf16x3(q->operands) ? cs_conv_fwd_b3(q, st) : cs_conv_fwd_h2(q, st);
}

int bwd_data(const catseg_conv_bwd_data_desc* q, hipStream_t st) {
  CS_REQUIRE(q != nullptr, "null descriptor");
  if (int e = check_operands(q->operands, q->dy_scale, q->w_scale)) return e;
  CS_REQUIRE(q->operands != CATSEG_OPERANDS_F16X2, "planar f16x2 operands are for backward-weight only");
  return q->operands == CATSEG_OPERANDS_F32 ? cs_conv_bwd_data_f32(q, st) : is_bf16x3(q->operands) ? cs_conv_bwd_data_b3(q, st) : cs_conv_bwd_data_h2(q, st);
}

int bwd_weight(const catseg_conv_bwd_weight_desc* q, hipStream_t st) {
  CS_REQUIRE(q != nullptr, "null descriptor");
  if (int e = check_operands(q->operands, q->x_scale, q->dy_scale)) return e;
  CS_REQUIRE(q->operands != CATSEG_OPERANDS_BF16X3_BLOCKED, "blocked bf16x3 operands are for forward and backward-data only");
  CS_REQUIRE(q->operands == CATSEG_OPERANDS_F32 || q->dbias == nullptr, "dbias needs fp32 operands (catseg_bias_grad computes it on its own)");
  return q->operands == CATSEG_OPERANDS_F32 ? cs_conv_bwd_weight_f32(q, st) : is_bf16x3(q->operands) ? cs_conv_bwd_weight_b3(q, st) : cs_conv_bwd_weight_h2(q, st);
}

}  // namespace

extern "C" int catseg_conv2d_fwd(const catseg_conv_fwd_desc* d, catseg_stream_t stream) { return named(__func__, fwd(d, (hipStream_t)stream)); }
extern "C" int catseg_conv2d_bwd_data(const catseg_conv_bwd_data_desc* d, catseg_stream_t stream) {
  return named(__func__, bwd_data(d, (hipStream_t)stream));
}
extern "C" int catseg_conv2d_bwd_weight(const catseg_conv_bwd_weight_desc* d, catseg_stream_t stream) {
  return named(__func__, bwd_weight(d, (hipStream_t)stream));
}
// fp32: split-reduction slabs or the direct kernel's, + the bias-gradient partials; planes: the slabs, only when more than one split is planned.
// 0 for a geometry or a form no backward-weight takes.
extern "C" size_t catseg_conv2d_bwd_weight_workspace(const catseg_conv_desc* geo, int operands) {
  if (geo == nullptr || operands < CATSEG_OPERANDS_F32 || operands > CATSEG_OPERANDS_F16X2_BLOCKED || operands == CATSEG_OPERANDS_BF16X3_BLOCKED) return 0;
  return operands == CATSEG_OPERANDS_F32 ? cs_conv_bwd_weight_workspace_f32(geo) : cs_wgrad_plan(geo).workspace_bytes;
}
