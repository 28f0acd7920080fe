// kt_throttle_batch.cpp — the shape checks of a throttle batch, before anything of it is stored.  A kt_snapshot is a struct of
// pointers and counts that nothing ties to each other: a slice in the wrong position, an operator byte that is none, offsets that
// run backwards would reach the index builder as a selector nobody wrote (or as reads far outside the caller's arrays).  Every
// feed path of throttles — kt_upsert_throttles, kt_upsert_throttle, kt_load_snapshot — runs this one pass over the WHOLE batch
// first; kt_validate_throttles is the same pass without an engine.  No HIP, no engine object: this file compiles on its own.
#include "kt_throttle_batch.h"

#include <cstdarg>
#include <cstdio>

namespace kt {
namespace {

struct Refusal {
  char* err;
  size_t err_len;
  __attribute__((format(printf, 3, 4))) int32_t operator()(int32_t code, const char* fmt, ...) const {
    if (err && err_len > 0) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(err, err_len, fmt, ap);
      va_end(ap);
    }
    return code;
  }
  // one array of the batch does not fit the others
  int32_t bad(const char* what, long long i, long long v) const {
    return (*this)(KT_ERR_INVALID_ARGUMENT, "kt_upsert_throttles: %s[%lld] = %lld does not fit the other arguments", what, i, v);
  }
  int32_t null(const char* what) const { return (*this)(KT_ERR_INVALID_ARGUMENT, "kt_upsert_throttles: %s is NULL", what); }
};

constexpr uint64_t kBound = 1ull << 60;  // |value| beyond it: KT_ERR_OVERFLOW_RISK (the engine's kSumBound)

uint64_t uabs64(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// row i of an amount table as amount_from_table reads it: values only under their presence bits, the count only under has_count
bool amount_in_bound(const kt_amounts& a, size_t i, int D) {
  const uint32_t present = a.present ? a.present[i] : 0u;
  for (int d = 0; d < D; ++d)
    if (((present >> d) & 1u) && uabs64(a.v[i * (size_t)D + d]) > kBound) return false;
  return !(a.has_count && a.has_count[i] && uabs64(a.count[i]) > kBound);
}

}  // namespace

int32_t validate_throttle_batch(const kt_snapshot* b, const int32_t* rows, int32_t n_dims, int32_t throttle_capacity,
                                int32_t namespace_capacity, char* err, size_t err_len) {
  const Refusal no{err, err_len};
  if (err && err_len > 0) err[0] = 0;
  if (!b) return no.null("batch");
  if (n_dims < 1 || n_dims > KT_MAX_DIMS) return no(KT_ERR_INVALID_ARGUMENT, "n_dims = %d", n_dims);
  const int32_t n = b->n_thr;
  if (n < 0) return no(KT_ERR_INVALID_ARGUMENT, "kt_upsert_throttles: n_thr = %d", n);
  if (n == 0) return KT_OK;  // (a batch without throttles: its D and its other sections are not looked at)
  const int D = n_dims;
  if (b->D != D) return no(KT_ERR_INVALID_ARGUMENT, "batch D=%d, engine D=%d", b->D, D);
  if (!b->thr_flags) return no.null("thr_flags");
  if (!b->thr_ns) return no.null("thr_ns");
  if (!b->thr_thrl_flag || !b->thr_thrl_has) return no.null("thr_thrl_flag / thr_thrl_has");
  if (!b->thr_status_msgs_fp || !b->thr_spec_msgs_fp) return no.null("thr_status_msgs_fp / thr_spec_msgs_fp");
  if (!b->thr_ovr_off) return no.null("thr_ovr_off");
  if (!b->thr_term_off) return no.null("thr_term_off");
  // ---- rows and namespace ids, at every position of the batch
  for (int32_t i = 0; i < n; ++i) {
    const int32_t row = rows ? rows[i] : i;
    if (row < 0 || row >= throttle_capacity) return no(KT_ERR_OUT_OF_RANGE, "throttle row %d", row);
    if (!(b->thr_flags[i] & KT_THR_CLUSTER) && b->thr_ns[i] >= (uint32_t)(namespace_capacity < 0 ? 0 : namespace_capacity))
      return no(KT_ERR_OUT_OF_RANGE, "throttle %d: namespace id %u", i, b->thr_ns[i]);
  }
  // ---- the offsets per throttle: they start at 0 and never decrease; their last entries are the counts of everything below
  if (b->thr_ovr_off[0] != 0u) return no.bad("thr_ovr_off", 0, b->thr_ovr_off[0]);
  if (b->thr_term_off[0] != 0u) return no.bad("thr_term_off", 0, b->thr_term_off[0]);
  for (int32_t i = 0; i < n; ++i) {
    if (b->thr_ovr_off[i + 1] < b->thr_ovr_off[i]) return no.bad("thr_ovr_off", i + 1, b->thr_ovr_off[i + 1]);
    if (b->thr_term_off[i + 1] < b->thr_term_off[i]) return no.bad("thr_term_off", i + 1, b->thr_term_off[i + 1]);
  }
  const uint32_t n_ovr = b->thr_ovr_off[n], n_term = b->thr_term_off[n];
  // ---- masks name dimensions below n_dims (a value array under a presence bit must exist)
  const uint32_t dmask = D >= 32 ? ~0u : (1u << D) - 1u;
  struct Tab { const char* name; const kt_amounts* a; };
  const Tab tabs[4] = {{"thr_spec.present", &b->thr_spec}, {"thr_calc.present", &b->thr_calc}, {"thr_used.present", &b->thr_used},
                       {"thr_reserved.present", &b->thr_reserved}};
  auto amount_shape = [&](const char* name, const kt_amounts& a, uint32_t i) -> int32_t {
    const uint32_t present = a.present ? a.present[i] : 0u;
    if (present & ~dmask) return no.bad(name, i, present);
    if (present && !a.v) return no.null(name);
    if (a.has_count && a.has_count[i] && !a.count) return no.null(name);
    return KT_OK;
  };
  for (int32_t i = 0; i < n; ++i) {
    for (const Tab& t : tabs)
      if (int32_t rc = amount_shape(t.name, *t.a, (uint32_t)i)) return rc;
    if ((b->thr_thrl_has[i] | b->thr_thrl_flag[i]) & ~dmask)
      return no.bad("thr_thrl_has | thr_thrl_flag", i, b->thr_thrl_has[i] | b->thr_thrl_flag[i]);
  }
  if (n_ovr > 0) {
    if (!b->ovr_begin_s || !b->ovr_begin_ns || !b->ovr_end_s || !b->ovr_end_ns || !b->ovr_flags) return no.null("ovr_begin_* / ovr_end_* / ovr_flags");
    for (uint32_t o = 0; o < n_ovr; ++o)
      if (int32_t rc = amount_shape("ovr_thr.present", b->ovr_thr, o)) return rc;
  }
  // ---- selector terms: known flags, requirement ranges that start at 0, never decrease and end inside the pools
  if (n_term > 0) {
    if (!b->term_flags || !b->term_preq_off || !b->term_nreq_off) return no.null("term_flags / term_preq_off / term_nreq_off");
    if (b->term_preq_off[0] != 0u || b->term_nreq_off[0] != 0u)
      return no.bad("term_preq_off / term_nreq_off", 0, b->term_preq_off[0] | b->term_nreq_off[0]);
    for (uint32_t t = 0; t < n_term; ++t) {
      if (b->term_preq_off[t + 1] < b->term_preq_off[t]) return no.bad("term_preq_off", t + 1, b->term_preq_off[t + 1]);
      if (b->term_nreq_off[t + 1] < b->term_nreq_off[t]) return no.bad("term_nreq_off", t + 1, b->term_nreq_off[t + 1]);
      if (b->term_flags[t] & ~(KT_TERM_POD_SEL_INVALID | KT_TERM_NS_SEL_INVALID)) return no.bad("term_flags", t, b->term_flags[t]);
    }
    if (b->term_preq_off[n_term] > b->preq.n || b->term_nreq_off[n_term] > b->nreq.n)
      return no(KT_ERR_OUT_OF_RANGE, "selector terms reference %u / %u requirements, pools hold %u / %u", b->term_preq_off[n_term],
                b->term_nreq_off[n_term], b->preq.n, b->nreq.n);
  }
  // ---- the requirement pools: every operator is one of the four, value ranges start at 0 and never decrease (the values
  // themselves are pair ids of any size: kt_reqs carries no count of them, a non-empty range only needs the array)
  struct Pool { const char* op; const char* val_off; const kt_reqs* q; };
  const Pool pools[2] = {{"preq.op", "preq.val_off", &b->preq}, {"nreq.op", "nreq.val_off", &b->nreq}};
  for (const Pool& pl : pools) {
    const kt_reqs& q = *pl.q;
    if (q.n == 0) continue;
    if (!q.op || !q.key || !q.val_off) return no.null(pl.op);
    if (q.val_off[0] != 0u) return no.bad(pl.val_off, 0, q.val_off[0]);
    for (uint32_t r = 0; r < q.n; ++r) {
      if (q.op[r] > KT_OP_DOES_NOT_EXIST) return no.bad(pl.op, r, q.op[r]);
      if (q.val_off[r + 1] < q.val_off[r]) return no.bad(pl.val_off, r + 1, q.val_off[r + 1]);
    }
    if (q.val_off[q.n] > 0u && !q.val) return no.bad(pl.val_off, q.n, q.val_off[q.n]);
  }
  // ---- stored status and reservations stay inside the exact range
  for (int32_t i = 0; i < n; ++i)
    if (!amount_in_bound(b->thr_used, (size_t)i, D) || !amount_in_bound(b->thr_reserved, (size_t)i, D))
      return no(KT_ERR_OVERFLOW_RISK, "throttle %d: status.used / reserved beyond 2^60", i);
  return KT_OK;
}

}  // namespace kt

int32_t kt_validate_throttles(const kt_snapshot* batch, const int32_t* thr_rows, int32_t n_dims, int32_t throttle_capacity,
                              int32_t namespace_capacity, char* err, int32_t err_len) {
  return kt::validate_throttle_batch(batch, thr_rows, n_dims, throttle_capacity, namespace_capacity, err, err_len > 0 ? (size_t)err_len : 0);
}
