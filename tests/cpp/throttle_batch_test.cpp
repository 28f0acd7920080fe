// throttle_batch_test.cpp — kt::validate_throttle_batch (kt_throttle_batch.cpp), the validation pass of kt_upsert_throttles, on
// batches whose offsets point far outside their arrays: each must be refused, and refused without a read beyond what the counts and
// the offsets checked so far cover.  Every array lives in a heap block of exactly its size, so under tools/sanitize_host.sh
// (-fsanitize=address,undefined) one read too far is a report.  Host only: the translation unit is compiled in, it needs no HIP
// and no engine library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kt_throttle_batch.h"

static int g_fail = 0;

struct Pool {
  std::vector<uint8_t> op;
  std::vector<uint32_t> key, val_off{0}, val;
  bool null_val = false;
  void add(uint8_t o, uint32_t k, std::vector<uint32_t> vals) {
    op.push_back(o), key.push_back(k);
    val.insert(val.end(), vals.begin(), vals.end());
    val_off.push_back((uint32_t)val.size());
  }
  kt_reqs view() { return kt_reqs{(uint32_t)op.size(), op.data(), key.data(), val_off.data(), null_val ? nullptr : val.data()}; }
};

struct Amounts {
  std::vector<int64_t> v, count;
  std::vector<uint32_t> present;
  std::vector<uint8_t> has_count;
  Amounts(size_t n, int D) : v(n * D, 0), count(n, 0), present(n, 0), has_count(n, 0) {}
  kt_amounts view() { return kt_amounts{v.data(), present.data(), count.data(), has_count.data()}; }
};

// two throttles: a Throttle of namespace 0 with two terms and an override, a ClusterThrottle with one term
struct Batch {
  static constexpr int D = 4;
  std::vector<uint32_t> flags{KT_THR_VALID | KT_THR_RESPONSIBLE, KT_THR_VALID | KT_THR_RESPONSIBLE | KT_THR_CLUSTER}, ns{0, 0};
  Amounts spec{2, D}, calc{2, D}, used{2, D}, reserved{2, D}, ovr_thr{1, D};
  std::vector<uint32_t> thrl_flag{0, 0}, thrl_has{0, 0};
  std::vector<uint64_t> status_fp{0, 0}, spec_fp{0, 0};
  std::vector<uint32_t> ovr_off{0, 1, 1}, term_off{0, 2, 3};
  std::vector<int64_t> ovr_begin_s{100}, ovr_end_s{200};
  std::vector<int32_t> ovr_begin_ns{0}, ovr_end_ns{0};
  std::vector<uint8_t> ovr_flags{0}, term_flags{0, 0, 0};
  std::vector<uint32_t> term_preq_off{0, 1, 2, 3}, term_nreq_off{0, 0, 0, 1};
  Pool preq, nreq;
  std::vector<int32_t> rows{3, 1};
  Batch() {
    spec.present[0] = 0x3, spec.v[0] = 4000, spec.v[1] = 1 << 20;
    used.present[0] = 0x1, used.v[0] = 700;
    ovr_thr.present[0] = 0x1, ovr_thr.v[0] = 6000;
    preq.add(KT_OP_IN, 1, {1, 2});
    preq.add(KT_OP_EXISTS, 2, {});
    preq.add(KT_OP_NOT_IN, 3, {5});
    nreq.add(KT_OP_IN, 4, {7});
  }
  kt_snapshot view() {
    kt_snapshot b;
    memset(&b, 0, sizeof b);
    b.D = D, b.n_thr = (int32_t)flags.size();
    b.thr_flags = flags.data(), b.thr_ns = ns.data();
    b.thr_spec = spec.view(), b.thr_calc = calc.view(), b.thr_used = used.view(), b.thr_reserved = reserved.view();
    b.thr_thrl_flag = thrl_flag.data(), b.thr_thrl_has = thrl_has.data();
    b.thr_status_msgs_fp = status_fp.data(), b.thr_spec_msgs_fp = spec_fp.data();
    b.thr_ovr_off = ovr_off.data();
    b.ovr_begin_s = ovr_begin_s.data(), b.ovr_begin_ns = ovr_begin_ns.data(), b.ovr_end_s = ovr_end_s.data(), b.ovr_end_ns = ovr_end_ns.data();
    b.ovr_flags = ovr_flags.data(), b.ovr_thr = ovr_thr.view();
    b.thr_term_off = term_off.data(), b.term_flags = term_flags.data();
    b.term_preq_off = term_preq_off.data(), b.term_nreq_off = term_nreq_off.data();
    b.preq = preq.view(), b.nreq = nreq.view();
    return b;
  }
};

static void expect(const char* what, Batch& x, int32_t code, const char* text, int32_t thr_cap = 8, int32_t ns_cap = 2) {
  kt_snapshot b = x.view();
  char err[200];
  memset(err, 'x', sizeof err);
  const int32_t rc = kt::validate_throttle_batch(&b, x.rows.data(), Batch::D, thr_cap, ns_cap, err, sizeof err);
  const bool terminated = memchr(err, 0, sizeof err) != nullptr;
  if (rc != code || !terminated || (code == KT_OK ? err[0] != 0 : strstr(err, text) == nullptr)) {
    ++g_fail;
    printf("FAIL %s: code %d (expected %d), text \"%.*s\" (expected \"%s\")\n", what, rc, code, terminated ? 199 : 0, err, text);
  }
}

int main() {
  const uint32_t far = 1u << 31;
  { Batch x; expect("the valid batch", x, KT_OK, ""); }
  { Batch x; x.rows = {5, 5}; expect("one row twice", x, KT_OK, ""); }
  { Batch x; x.rows = {1, 8}; expect("the last entry's row at the capacity", x, KT_ERR_OUT_OF_RANGE, "throttle row 8"); }
  { Batch x; x.ns[0] = 2; expect("a namespace id at the capacity", x, KT_ERR_OUT_OF_RANGE, "throttle 0: namespace id 2"); }
  { Batch x; x.ns[1] = far; expect("a ClusterThrottle's namespace id is not looked at", x, KT_OK, ""); }
  // offsets per throttle that run backwards behind a jump far outside the arrays below them
  { Batch x; x.term_off = {0, far, 3}; expect("thr_term_off jumps to 2^31 and back", x, KT_ERR_INVALID_ARGUMENT, "thr_term_off[2] = 3"); }
  { Batch x; x.ovr_off = {0, far, 1}; expect("thr_ovr_off jumps to 2^31 and back", x, KT_ERR_INVALID_ARGUMENT, "thr_ovr_off[2] = 1"); }
  { Batch x; x.term_off = {1, 2, 3}; expect("thr_term_off starts at 1", x, KT_ERR_INVALID_ARGUMENT, "thr_term_off[0] = 1"); }
  { Batch x; x.term_off = {0, 3, 1}; expect("thr_term_off backwards", x, KT_ERR_INVALID_ARGUMENT, "thr_term_off[2] = 1"); }
  // requirement ranges of the terms
  { Batch x; x.term_preq_off = {0, far, 2, 3}; expect("term_preq_off jumps to 2^31 and back", x, KT_ERR_INVALID_ARGUMENT, "term_preq_off[2] = 2"); }
  { Batch x; x.term_preq_off = {0, 1, 2, far}; expect("term_preq_off[n] = 2^31, the pool holds 3", x, KT_ERR_OUT_OF_RANGE, "selector terms reference 2147483648 / 1 requirements, pools hold 3 / 1"); }
  { Batch x; x.term_preq_off = {0, 1, 2, 4}; expect("term_preq_off[n] one beyond the pool", x, KT_ERR_OUT_OF_RANGE, "selector terms reference 4 / 1"); }
  { Batch x; x.term_nreq_off = {0, 0, 0, far}; expect("term_nreq_off[n] = 2^31, the pool holds 1", x, KT_ERR_OUT_OF_RANGE, "pools hold 3 / 1"); }
  { Batch x; x.term_nreq_off = {0, far, far - 1, 1}; expect("term_nreq_off backwards", x, KT_ERR_INVALID_ARGUMENT, "term_nreq_off[2]"); }
  { Batch x; x.term_nreq_off = {7, 7, 7, 7}; expect("term_nreq_off starts at 7", x, KT_ERR_INVALID_ARGUMENT, "term_preq_off / term_nreq_off[0] = 7"); }
  // value ranges of the requirements: kt_reqs carries no count of the values, they are never read — a tail of 2^31 is refused by
  // what follows it (a decrease) or by the missing array
  { Batch x; x.preq.val_off = {0, far, 2, 3}; expect("preq.val_off jumps to 2^31 and back", x, KT_ERR_INVALID_ARGUMENT, "preq.val_off[2] = 2"); }
  { Batch x; x.nreq.val_off = {0, far}; x.nreq.null_val = true; expect("nreq.val_off ends at 2^31 without a value array", x, KT_ERR_INVALID_ARGUMENT, "nreq.val_off[1] = 2147483648"); }
  { Batch x; x.preq.val_off = {far, far, far, far}; expect("preq.val_off starts at 2^31", x, KT_ERR_INVALID_ARGUMENT, "preq.val_off[0] = 2147483648"); }
  { Batch x; x.preq.val_off = {0, 2, 2, far}; expect("a value range of 2^31 entries is shape enough: the values are not read", x, KT_OK, ""); }
  // operators, flags, masks, the bound
  { Batch x; x.preq.op[2] = 4; expect("operator 4", x, KT_ERR_INVALID_ARGUMENT, "preq.op[2] = 4"); }
  { Batch x; x.term_flags[2] = 0x80; expect("term flag 0x80", x, KT_ERR_INVALID_ARGUMENT, "term_flags[2] = 128"); }
  { Batch x; x.calc.present[1] = 1u << Batch::D; expect("a mask bit at n_dims", x, KT_ERR_INVALID_ARGUMENT, "thr_calc.present[1] = 16"); }
  { Batch x; x.ovr_thr.present[0] = 0x80000000u; expect("an override's mask bit 31", x, KT_ERR_INVALID_ARGUMENT, "ovr_thr.present[0]"); }
  { Batch x; x.thrl_has[1] = 0x10; expect("a throttled key at n_dims", x, KT_ERR_INVALID_ARGUMENT, "thr_thrl_has | thr_thrl_flag[1] = 16"); }
  { Batch x; x.used.v[1] = INT64_MIN; expect("a value beyond 2^60 without its presence bit is not looked at", x, KT_OK, ""); }
  { Batch x; x.used.v[0] = INT64_MIN; expect("status.used = INT64_MIN", x, KT_ERR_OVERFLOW_RISK, "throttle 0: status.used / reserved beyond 2^60"); }
  { Batch x; x.reserved.count[1] = (1ll << 60) + 1, x.reserved.has_count[1] = 1; expect("reserved pods beyond 2^60", x, KT_ERR_OVERFLOW_RISK, "throttle 1"); }
  {  // another D; a batch without throttles is not looked at; the text fits a buffer of any size
    Batch x;
    kt_snapshot b = x.view();
    char err[8];
    if (kt::validate_throttle_batch(&b, nullptr, Batch::D + 1, 8, 2, err, sizeof err) != KT_ERR_INVALID_ARGUMENT || strcmp(err, "batch D") != 0)
      ++g_fail, printf("FAIL another D: \"%s\"\n", err);
    if (kt::validate_throttle_batch(&b, nullptr, Batch::D, 8, 2, nullptr, 0) != KT_OK) ++g_fail, printf("FAIL no text buffer\n");
    kt_snapshot none;
    memset(&none, 0, sizeof none);
    none.D = 9;
    if (kt::validate_throttle_batch(&none, nullptr, Batch::D, 8, 2, err, sizeof err) != KT_OK) ++g_fail, printf("FAIL no throttles\n");
    if (kt_validate_throttles(&b, x.rows.data(), Batch::D, 3, 2, err, (int32_t)sizeof err) != KT_ERR_OUT_OF_RANGE) ++g_fail, printf("FAIL the exported call\n");
  }
  if (g_fail) {
    printf("throttle_batch_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("throttle_batch_test: ok\n");
  return 0;
}
