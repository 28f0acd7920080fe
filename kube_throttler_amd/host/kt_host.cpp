#include <mutex>
#include <set>
// kt_host.cpp — see kt_host.hpp.  Host-side mirror of pkg/scheduler_plugin/plugin.go over the C-ABI.
#include "kt_host.hpp"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <ctime>

namespace kth {

const char* const PluginName = "kube-throttler";

// =====================================================================================================
// resource.Quantity
// =====================================================================================================
namespace {
__int128 pow10_128(int e) {
  __int128 r = 1;
  while (e-- > 0) r *= 10;
  return r;
}
}  // namespace

bool ParseQuantity(const std::string& text, Quantity* out, std::string* err) {
  // <quantity> ::= [+-]? digits[.digits]? | [+-]? .digits   followed by  Ki|Mi|Gi|Ti|Pi|Ei | n|u|m|""|k|M|G|T|P|E | e[+-]?N
  size_t i = 0;
  const size_t n = text.size();
  bool neg = false;
  if (i < n && (text[i] == '+' || text[i] == '-')) neg = text[i++] == '-';
  __int128 mant = 0;
  int frac_digits = 0, digits = 0;
  while (i < n && std::isdigit((unsigned char)text[i])) mant = mant * 10 + (text[i++] - '0'), ++digits;
  if (i < n && text[i] == '.') {
    ++i;
    while (i < n && std::isdigit((unsigned char)text[i])) mant = mant * 10 + (text[i++] - '0'), ++digits, ++frac_digits;
  }
  if (digits == 0 || digits > 36) {
    if (err) *err = "quantities must match the regular expression '^([+-]?[0-9.]+)([eEinumkKMGTP]*[-+]?[0-9]*)$'";
    return false;
  }
  const std::string suf = text.substr(i);
  int bin = -1, dec = 0;
  static const char* kBin[] = {"Ki", "Mi", "Gi", "Ti", "Pi", "Ei"};
  for (int k = 0; k < 6; ++k)
    if (suf == kBin[k]) bin = 10 * (k + 1);
  if (bin < 0) {
    if (suf == "n") dec = -9;
    else if (suf == "u") dec = -6;
    else if (suf == "m") dec = -3;
    else if (suf.empty()) dec = 0;
    else if (suf == "k") dec = 3;
    else if (suf == "M") dec = 6;
    else if (suf == "G") dec = 9;
    else if (suf == "T") dec = 12;
    else if (suf == "P") dec = 15;
    else if (suf == "E") dec = 18;
    else if ((suf[0] == 'e' || suf[0] == 'E') && suf.size() > 1) {
      size_t j = 1;
      bool eneg = false;
      if (suf[j] == '+' || suf[j] == '-') eneg = suf[j++] == '-';
      if (j >= suf.size()) { if (err) *err = "unable to parse quantity's suffix"; return false; }
      int ev = 0;
      for (; j < suf.size(); ++j) {
        if (!std::isdigit((unsigned char)suf[j]) || ev > 100) { if (err) *err = "unable to parse quantity's suffix"; return false; }
        ev = ev * 10 + (suf[j] - '0');
      }
      dec = eneg ? -ev : ev;
    } else {
      if (err) *err = "unable to parse quantity's suffix";
      return false;
    }
  }
  // value = mant * 10^-frac * (2^bin | 10^dec); in nano units: * 10^9
  __int128 num = mant;
  int exp10 = 9 - frac_digits + (bin < 0 ? dec : 0);
  if (bin >= 0) num <<= bin;
  __int128 nano;
  if (exp10 >= 0) {
    if (exp10 > 30) { if (err) *err = "quantity out of range"; return false; }
    nano = num * pow10_128(exp10);
  } else {
    if (-exp10 > 36) { nano = num != 0 ? 1 : 0; }
    else {
      const __int128 d = pow10_128(-exp10);
      nano = num / d;
      if (num % d != 0) nano += 1;  // round away from zero (magnitude; sign applied below)
    }
  }
  out->nano = neg ? -nano : nano;
  out->format = bin >= 0 ? Format::BinarySI
                         : (!suf.empty() && (suf[0] == 'e' || (suf[0] == 'E' && suf.size() > 1))) ? Format::DecimalExponent
                                                                                                   : Format::DecimalSI;
  return true;
}

bool ScaledValue(const Quantity& q, int scale, int64_t* out) {
  // value / 10^scale = nano * 10^(-9 - scale)
  const int e = -9 - scale;
  __int128 v = q.nano;
  if (e >= 0) {
    if (e > 18) return false;
    v *= pow10_128(e);
  } else {
    const __int128 d = pow10_128(-e);
    if (v % d != 0) return false;
    v /= d;
  }
  if (v > (__int128)INT64_MAX || v < (__int128)INT64_MIN) return false;
  *out = (int64_t)v;
  return true;
}

std::string FormatDecimalSI(const Quantity& q) {
  if (q.nano == 0) return "0";
  static const struct { int e; const char* s; } kSuf[] = {{27, "E"}, {24, "P"}, {21, "T"}, {18, "G"}, {15, "M"}, {12, "k"},
                                                          {9, ""},   {6, "m"},  {3, "u"},  {0, "n"}};
  for (auto& sf : kSuf) {
    const __int128 d = pow10_128(sf.e);
    if (q.nano % d == 0) {
      __int128 v = q.nano / d;
      const bool neg = v < 0;
      if (neg) v = -v;
      std::string digits;
      do { digits.insert(digits.begin(), (char)('0' + (int)(v % 10))); v /= 10; } while (v > 0);
      return (neg ? "-" : "") + digits + sf.s;
    }
  }
  return "?";
}

namespace {
std::string digits_of(__int128 v) {
  const bool neg = v < 0;
  if (neg) v = -v;
  std::string digits;
  do { digits.insert(digits.begin(), (char)('0' + (int)(v % 10))); v /= 10; } while (v > 0);
  return (neg ? "-" : "") + digits;
}
}  // namespace

std::string FormatQuantity(const Quantity& q) {
  if (q.nano == 0) return "0";
  Format f = q.format;
  const __int128 one = pow10_128(9);
  if (f == Format::BinarySI) {
    const __int128 mag = q.nano < 0 ? -q.nano : q.nano;
    if (mag < 1024 * one || q.nano % one != 0) f = Format::DecimalSI;  // small or fractional: shown as DecimalSI
  }
  if (f == Format::BinarySI) {
    static const char* kBin[] = {"", "Ki", "Mi", "Gi", "Ti", "Pi", "Ei"};
    __int128 v = q.nano / one;
    int e = 0;
    while (e < 6 && v % 1024 == 0) v /= 1024, ++e;
    return digits_of(v) + kBin[e];
  }
  if (f == Format::DecimalSI) return FormatDecimalSI(q);
  // DecimalExponent: mantissa without factors of 10, then the exponent lowered to a multiple of 3
  __int128 v = q.nano;
  int e = -9;
  while (v % 10 == 0) v /= 10, ++e;
  int r = ((e % 3) + 3) % 3;
  for (; r > 0; --r) v *= 10, --e;
  return e == 0 ? digits_of(v) : digits_of(v) + "e" + std::to_string(e);
}

std::map<std::string, std::string> ThrottleStatus::UsedStrings() const {
  std::map<std::string, std::string> out;
  for (auto& kv : used) out[kv.first] = FormatQuantity(kv.second);
  return out;
}

bool StatusSemanticEqual(const ThrottleStatus& a, const ThrottleStatus& b) {
  if (a.usedHasCounts != b.usedHasCounts || (a.usedHasCounts && a.usedPod != b.usedPod)) return false;
  if (a.throttledPod != b.throttledPod || a.throttledRequests != b.throttledRequests) return false;
  if (a.used.size() != b.used.size()) return false;
  for (auto& kv : a.used) {
    auto it = b.used.find(kv.first);
    if (it == b.used.end() || it->second.nano != kv.second.nano) return false;  // Format is not part of Cmp
  }
  return true;
}

// =====================================================================================================
// RFC3339
// =====================================================================================================
namespace {
int64_t days_from_civil(int64_t y, unsigned m, unsigned d) {  // proleptic Gregorian, days since 1970-01-01
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const unsigned yoe = (unsigned)(y - era * 400);
  const unsigned doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (int64_t)doe - 719468;
}
bool num(const std::string& s, size_t pos, size_t len, int* out) {
  if (pos + len > s.size()) return false;
  int v = 0;
  for (size_t i = 0; i < len; ++i) {
    if (!std::isdigit((unsigned char)s[pos + i])) return false;
    v = v * 10 + (s[pos + i] - '0');
  }
  *out = v;
  return true;
}
}  // namespace

bool ParseRFC3339(const std::string& t, int64_t* sec, int32_t* nsec, std::string* err) {
  auto fail = [&]() {
    if (err) *err = "parsing time \"" + t + "\" as \"2006-01-02T15:04:05Z07:00\": cannot parse";
    return false;
  };
  int Y, M, D, h, m, s;
  if (!num(t, 0, 4, &Y) || t.size() < 20 || t[4] != '-' || !num(t, 5, 2, &M) || t[7] != '-' || !num(t, 8, 2, &D) ||
      (t[10] != 'T' && t[10] != 't') || !num(t, 11, 2, &h) || t[13] != ':' || !num(t, 14, 2, &m) || t[16] != ':' ||
      !num(t, 17, 2, &s))
    return fail();
  static const int kDays[] = {31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  if (M < 1 || M > 12 || D < 1 || D > kDays[M - 1] || h > 23 || m > 59 || s > 59) return fail();
  if (M == 2 && D == 29 && !((Y % 4 == 0 && Y % 100 != 0) || Y % 400 == 0)) return fail();
  size_t i = 19;
  int64_t ns = 0;
  if (t[i] == '.' || t[i] == ',') {
    ++i;
    int nd = 0;
    while (i < t.size() && std::isdigit((unsigned char)t[i])) {
      if (nd < 9) ns = ns * 10 + (t[i] - '0'), ++nd;
      ++i;
    }
    if (nd == 0) return fail();
    while (nd++ < 9) ns *= 10;
  }
  int64_t off = 0;
  if (i < t.size() && (t[i] == 'Z' || t[i] == 'z') && i + 1 == t.size()) {
  } else if (i + 6 == t.size() && (t[i] == '+' || t[i] == '-') && t[i + 3] == ':') {
    int oh, om;
    if (!num(t, i + 1, 2, &oh) || !num(t, i + 4, 2, &om) || oh > 23 || om > 59) return fail();
    off = (oh * 3600 + om * 60) * (t[i] == '+' ? 1 : -1);
  } else {
    return fail();
  }
  *sec = days_from_civil(Y, (unsigned)M, (unsigned)D) * 86400 + h * 3600 + m * 60 + s - off;
  *nsec = (int32_t)ns;
  return true;
}

// =====================================================================================================
// plugin
// =====================================================================================================
namespace {

bool valid_name_part(const std::string& s) {  // qualified-name "name" part: [A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?, <= 63
  if (s.empty() || s.size() > 63) return false;
  if (!std::isalnum((unsigned char)s.front()) || !std::isalnum((unsigned char)s.back())) return false;
  for (char c : s)
    if (!std::isalnum((unsigned char)c) && c != '-' && c != '_' && c != '.') return false;
  return true;
}
bool valid_label_key(const std::string& k) {
  const size_t slash = k.find('/');
  if (slash == std::string::npos) return valid_name_part(k);
  if (k.find('/', slash + 1) != std::string::npos) return false;
  const std::string prefix = k.substr(0, slash);
  if (prefix.empty() || prefix.size() > 253) return false;
  // DNS-1123 subdomain
  bool start = true;
  for (size_t i = 0; i < prefix.size(); ++i) {
    const char c = prefix[i];
    if (c == '.') {
      if (start || prefix[i - 1] == '-') return false;
      start = true;
      continue;
    }
    if (!(std::islower((unsigned char)c) || std::isdigit((unsigned char)c) || c == '-')) return false;
    if (start && c == '-') return false;
    start = false;
  }
  if (start || prefix.back() == '-') return false;
  return valid_name_part(k.substr(slash + 1));
}
bool valid_label_value(const std::string& v) { return v.empty() || valid_name_part(v); }
}  // namespace
// exported for the CPU cross-check against the Python restatement (objects.py)
bool ValidLabelKey(const std::string& k) { return valid_label_key(k); }
bool ValidLabelValue(const std::string& v) { return valid_label_value(v); }
namespace {

template <class K>
struct RowTable {  // key -> dense row with a free list
  std::unordered_map<K, int64_t> row_of;
  std::vector<int64_t> free_rows;
  int64_t next = 0, cap = 0;
  int64_t find(const K& k) const {
    auto it = row_of.find(k);
    return it == row_of.end() ? -1 : it->second;
  }
  int64_t acquire(const K& k) {
    int64_t r = find(k);
    if (r >= 0) return r;
    if (!free_rows.empty()) {
      r = free_rows.back();
      free_rows.pop_back();
    } else if (next < cap) {
      r = next++;
    } else {
      return -1;
    }
    row_of[k] = r;
    return r;
  }
  void release(const K& k) {
    auto it = row_of.find(k);
    if (it == row_of.end()) return;
    free_rows.push_back(it->second);
    row_of.erase(it);
  }
};

// more than KT_MAX_DIMS resource names: one engine per PAGE of KT_MAX_DIMS names (kt_paged_*); a name's values live at
// v[page * KT_MAX_DIMS + dimension], its presence bit in present[page]
constexpr int kMaxPages = 16;
struct DenseAmount {
  int64_t v[KT_MAX_DIMS * kMaxPages] = {0};
  uint32_t present[kMaxPages] = {0};
  int64_t count = 0;
  uint8_t has_count = 0;
};
// the count part of a throttle row's applied status (what a page created after a ReconcileAll has to be seeded with)
struct CountPart {
  bool set = false;
  int64_t used_count = 0, calc_count = 0;
  uint8_t used_has = 0, calc_has = 0, calc_at_nonzero = 0, thrl_pod = 0;
  uint64_t msgs_fp = 0;
};
struct DimRef {
  int page, dim, scale;
};

}  // namespace

struct KubeThrottler::Impl {
  // PreFilter / Reserve run on the scheduling goroutine, Unreserve on binding goroutines, the event handlers on informer
  // goroutines (plugin.go:148-257): every public method takes this lock (recursive: the methods call each other)
  std::recursive_mutex mu;
  PluginArgs args;
  kt_engine* e = nullptr;  // page 0
  std::vector<kt_engine*> pages;  // pages[0] == e; page k is created the first time a name does not fit pages 0..k-1
  kt_config cfg{};
  int D = KT_MAX_DIMS;
  std::map<std::string, DimRef> dims;  // resource name -> (page, dimension, scale)
  std::map<std::string, Namespace> ns_objs;  // Namespace objects seen (a page created later replays them)
  std::vector<CountPart> count_part;         // per throttle row
  std::vector<uint64_t> spec_fp;             // per throttle row: fingerprint of its override messages
  // resource name -> Format of the first non-zero quantity seen under that name: what a `used` sum inherits through
  // Quantity.Add when every pod writes the resource in one suffix family (the reference's result otherwise depends on
  // the lister's pod order)
  std::map<std::string, Format> dim_format;
  std::map<std::string, ThrottleStatus> written;  // thr_key -> status last handed to UpdateStatus
  std::unordered_map<std::string, uint32_t> key_ids;
  std::unordered_map<std::string, uint32_t> pair_ids;
  RowTable<std::string> ns_rows, pod_rows, thr_rows;
  std::vector<Throttle> thr_by_row;
  std::vector<uint8_t> thr_live;
  std::vector<std::vector<std::string>> thr_msgs;
  std::unordered_map<std::string, Pod> pods;
  // reserved cache: throttle row -> pod key -> amount of the pod (reserved_resource_amounts.go:32-41)
  std::map<int32_t, std::map<std::string, DenseAmount>> reserved;
  std::vector<uint8_t> last_status;
  int64_t last_row_pending = -1;  // pod row whose status row LastStatusOf still has to fetch (PreFilter allowed it on the summary)

  uint32_t key_id(const std::string& k) { return key_ids.emplace(k, (uint32_t)key_ids.size() + 1).first->second; }
  uint32_t pair_id(const std::string& k, const std::string& v) {
    std::string kv = k;
    kv.push_back('\0');
    kv += v;
    return pair_ids.emplace(kv, (uint32_t)pair_ids.size() + 1).first->second;
  }
  static std::string thr_key(const Throttle& t) { return (t.cluster ? "C:" : "T:") + t.Key(); }

  // a name's (page, dimension, scale); a name that fits no existing page opens the next one (add_page)
  bool dim_of(const std::string& name, DimRef* out, std::string* err) {
    auto it = dims.find(name);
    if (it == dims.end()) {
      const int page = (int)(dims.size() / (size_t)D);
      if (page >= kMaxPages) {
        if (err) *err = "more than " + std::to_string(D * kMaxPages) + " distinct resource names";
        return false;
      }
      if (page >= (int)pages.size() && !add_page(err)) return false;
      int sc = name == "cpu" ? -3 : 0;
      auto s = args.resourceScales.find(name);
      if (s != args.resourceScales.end()) sc = s->second;
      it = dims.emplace(name, DimRef{page, (int)(dims.size() % (size_t)D), sc}).first;
    }
    *out = it->second;
    return true;
  }
  bool register_names(const ResourceList& rl, std::string* err) {
    DimRef r;
    for (auto& kv : rl)
      if (!dim_of(kv.first, &r, err)) return false;
    return true;
  }
  bool register_names(const ResourceAmount& a, std::string* err) { return register_names(a.requests, err); }
  // page `page`'s values of a resource list (every name is parsed and checked, the other pages' names are skipped)
  bool fill_row(const ResourceList& rl, int page, int64_t* v, uint32_t* present, std::string* err) {
    for (auto& kv : rl) {
      Quantity q;
      DimRef r;
      if (!ParseQuantity(kv.second, &q, err) || !dim_of(kv.first, &r, err)) return false;
      int64_t x;
      if (!ScaledValue(q, r.scale, &x)) {
        if (err) *err = "quantity " + kv.second + " of " + kv.first + " is not representable at scale 1e" + std::to_string(r.scale);
        return false;
      }
      if (q.nano != 0) dim_format.emplace(kv.first, q.format);
      if (r.page != page) continue;
      v[r.dim] = x;
      *present |= 1u << r.dim;
    }
    return true;
  }
  bool fill_amount(const ResourceAmount& a, int page, DenseAmount* d, std::string* err) {
    *d = DenseAmount();
    d->has_count = a.hasCounts;
    d->count = a.hasCounts ? a.pod : 0;
    return fill_row(a.requests, page, d->v, &d->present[0], err);
  }
  std::string engine_error(int32_t rc) { return "kt: " + std::to_string(rc) + ": " + kt_last_error(e); }
  std::string engine_error(int32_t rc, kt_engine* pe) { return "kt: " + std::to_string(rc) + ": " + kt_last_error(pe); }

  // page = -1: every page
  bool push_reserved(int32_t row, std::string* err, int only_page = -1) {
    DenseAmount tot;
    auto it = reserved.find(row);
    if (it != reserved.end())
      for (auto& kv : it->second) {  // podResourceAmountMap.totalResoruceAmount (reserved_resource_amounts.go:148-156)
        tot.has_count = 1;
        tot.count += 1;
        for (size_t k = 0; k < pages.size(); ++k) tot.present[k] |= kv.second.present[k];
        for (size_t d = 0; d < (size_t)D * pages.size(); ++d) tot.v[d] += kv.second.v[d];
      }
    for (size_t k = 0; k < pages.size(); ++k) {
      if (only_page >= 0 && (int)k != only_page) continue;
      kt_amounts am{tot.v + k * (size_t)D, &tot.present[k], &tot.count, &tot.has_count};
      int32_t rc = kt_set_reserved(pages[k], 1, &row, &am);
      if (rc != KT_OK) {
        if (err) *err = engine_error(rc, pages[k]);
        return false;
      }
    }
    return true;
  }
  // ResourceAmountOfPod of pod rows as the engines hold them (every page its own names)
  int32_t fetch_pod_amounts(int64_t n, const int64_t* rows, std::vector<DenseAmount>* out) {
    out->assign((size_t)n, DenseAmount());
    std::vector<int64_t> v((size_t)n * (size_t)D);
    std::vector<uint32_t> pr((size_t)n);
    for (size_t k = 0; k < pages.size(); ++k) {
      int32_t rc = kt_fetch_pod_requests(pages[k], n, rows, v.data(), pr.data());
      if (rc != KT_OK) return rc;
      for (int64_t i = 0; i < n; ++i) {
        std::memcpy((*out)[(size_t)i].v + k * (size_t)D, &v[(size_t)i * D], sizeof(int64_t) * (size_t)D);
        (*out)[(size_t)i].present[k] = pr[(size_t)i];
      }
    }
    for (auto& a : *out) a.has_count = 1, a.count = 1;
    return KT_OK;
  }

  bool upsert_namespace(size_t k, const std::string& name, int32_t row, std::string* err);
  bool upsert_pod(size_t k, const Pod& pod, int64_t row, uint32_t ns32, std::string* err);
  bool upsert_throttle(size_t k, const Throttle& thr, int32_t row, uint32_t ns32, std::vector<std::string>* msgs, uint64_t* fp,
                       std::string* err);
  bool add_page(std::string* err);
};

KubeThrottler::~KubeThrottler() {
  if (!p_) return;
  for (kt_engine* pe : p_->pages) kt_engine_destroy(pe);
}

std::unique_ptr<KubeThrottler> NewPlugin(const PluginArgs& args, std::string* err) {
  // DecodePluginArgs (plugin_args.go:46-51)
  if (args.name.empty()) {
    if (err) *err = "Name must not be empty";
    return nullptr;
  }
  if (args.targetSchedulerName.empty()) {
    if (err) *err = "TargetSchedulerName must not be empty";
    return nullptr;
  }
  std::unique_ptr<KubeThrottler> k(new KubeThrottler());
  k->p_.reset(new KubeThrottler::Impl());
  auto& p = *k->p_;
  p.args = args;
  kt_config& cfg = p.cfg;
  cfg.n_dims = p.D;
  cfg.max_labels = args.maxLabels;
  cfg.pod_capacity = args.podCapacity;
  cfg.throttle_capacity = args.throttleCapacity;
  cfg.namespace_capacity = args.namespaceCapacity;
  cfg.device = -1;
  cfg.kernel_variant = 0;
  int32_t rc = kt_engine_create(&cfg, &p.e);
  if (rc != KT_OK) {
    if (err) *err = std::string("kt_engine_create: ") + std::to_string(rc) + ": " + kt_last_error(nullptr);
    return nullptr;
  }
  p.pages.push_back(p.e);
  p.ns_rows.cap = args.namespaceCapacity;
  p.pod_rows.cap = args.podCapacity;
  p.thr_rows.cap = args.throttleCapacity;
  p.thr_by_row.resize((size_t)args.throttleCapacity);
  p.thr_live.assign((size_t)args.throttleCapacity, 0);
  p.thr_msgs.resize((size_t)args.throttleCapacity);
  p.count_part.resize((size_t)args.throttleCapacity);
  p.spec_fp.assign((size_t)args.throttleCapacity, 0);
  for (auto& kv : args.resourceScales) {
    DimRef r;
    if (!p.dim_of(kv.first, &r, err)) return nullptr;
  }
  return k;
}

// ---------------------------------------------------------------------------------------------------
// pages: one engine per KT_MAX_DIMS resource names, every page fed every namespace, pod and throttle
// ---------------------------------------------------------------------------------------------------
bool KubeThrottler::Impl::upsert_namespace(size_t k, const std::string& name, int32_t row, std::string* err) {
  auto it = ns_objs.find(name);
  std::vector<uint32_t> keys, pairs;
  if (it != ns_objs.end())
    for (auto& kv : it->second.labels) keys.push_back(key_id(kv.first)), pairs.push_back(pair_id(kv.first, kv.second));
  uint32_t off[2] = {0, (uint32_t)keys.size()};
  // the Namespace OBJECT is gone (or was never seen): the id stays (pods may still reference it), marked invalid
  uint8_t valid = it != ns_objs.end() ? 1 : 0;
  keys.push_back(0), pairs.push_back(0);
  kt_snapshot b{};
  b.D = D;
  b.n_ns = 1;
  b.ns_valid = &valid;
  b.ns_label_off = off;
  b.ns_label_key = keys.data();
  b.ns_label_pair = pairs.data();
  int32_t rc = kt_upsert_namespaces(pages[k], &b, &row);
  if (rc != KT_OK) { if (err) *err = engine_error(rc, pages[k]); return false; }
  return true;
}

bool KubeThrottler::Impl::upsert_pod(size_t k, const Pod& pod, int64_t row, uint32_t ns32, std::string* err) {
  std::vector<uint32_t> keys, pairs;
  for (auto& kv : pod.labels) keys.push_back(key_id(kv.first)), pairs.push_back(pair_id(kv.first, kv.second));
  uint32_t loff[2] = {0, (uint32_t)keys.size()};
  keys.push_back(0), pairs.push_back(0);
  const size_t nc = pod.containers.size() + pod.initContainers.size();
  std::vector<uint8_t> c_init(nc + 1, 0);
  std::vector<uint32_t> c_present(nc + 1, 0);
  std::vector<int64_t> c_req((nc + 1) * D, 0);
  size_t c = 0;
  for (auto& ic : pod.initContainers) {
    c_init[c] = 1;
    if (!fill_row(ic.requests, (int)k, &c_req[c * D], &c_present[c], err)) return false;
    ++c;
  }
  for (auto& ct : pod.containers) {
    if (!fill_row(ct.requests, (int)k, &c_req[c * D], &c_present[c], err)) return false;
    ++c;
  }
  uint32_t coff[2] = {0, (uint32_t)nc};
  std::vector<int64_t> ovh(D, 0);
  uint32_t ovh_present = 0;
  if (pod.hasOverhead) {
    if (!fill_row(pod.overhead, (int)k, ovh.data(), &ovh_present, err)) return false;
    ovh_present |= 0x80000000u;
  }
  uint32_t flags = KT_POD_VALID;
  if (pod.schedulerName == args.targetSchedulerName) flags |= KT_POD_SCHED_MATCH;
  if (!pod.nodeName.empty()) flags |= KT_POD_SCHEDULED;
  if (pod.phase == "Succeeded" || pod.phase == "Failed") flags |= KT_POD_FINISHED;
  kt_snapshot b{};
  b.D = D;
  b.L = args.maxLabels;
  b.n_pods = 1;
  b.pod_ns = &ns32;
  b.pod_flags = &flags;
  b.pod_label_off = loff;
  b.pod_label_key = keys.data();
  b.pod_label_pair = pairs.data();
  b.pod_ctr_off = coff;
  b.ctr_init = c_init.data();
  b.ctr_present = c_present.data();
  b.ctr_req = c_req.data();
  b.pod_ovh_present = &ovh_present;
  b.pod_ovh = ovh.data();
  int32_t rc = kt_upsert_pods(pages[k], &b, &row);
  if (rc != KT_OK) { if (err) *err = engine_error(rc, pages[k]); return false; }
  return true;
}

namespace {
struct ReqPool {
  std::vector<uint8_t> op;
  std::vector<uint32_t> key, val_off{0}, val;
  void add(uint8_t o, uint32_t k, const std::vector<uint32_t>& vals) {
    op.push_back(o);
    key.push_back(k);
    val.insert(val.end(), vals.begin(), vals.end());
    val_off.push_back((uint32_t)val.size());
  }
  kt_reqs view() {
    if (op.empty()) op.push_back(0), key.push_back(0);
    if (val.empty()) val.push_back(0);
    kt_reqs r;
    r.n = (uint32_t)(val_off.size() - 1);
    r.op = op.data();
    r.key = key.data();
    r.val_off = val_off.data();
    r.val = val.data();
    return r;
  }
};
}  // namespace

// msgs / fp (nullable): the reference's override messages and their fingerprint (the same for every page)
bool KubeThrottler::Impl::upsert_throttle(size_t k, const Throttle& thr, int32_t r32, uint32_t ns32, std::vector<std::string>* msgs_out,
                                          uint64_t* fp_out, std::string* err) {
  DenseAmount spec;
  if (!fill_amount(thr.threshold, (int)k, &spec, err)) return false;
  // overrides: parse instants once; unparsable ones are flagged and produce the reference's messages
  const size_t no = thr.overrides.size();
  std::vector<int64_t> ob(no + 1, KT_ZERO_TIME_S), oe(no + 1, KT_ZERO_TIME_S), ov((no + 1) * D, 0), ocount(no + 1, 0);
  std::vector<int32_t> obn(no + 1, 0), oen(no + 1, 0);
  std::vector<uint8_t> oflags(no + 1, 0), ohas(no + 1, 0);
  std::vector<uint32_t> opresent(no + 1, 0);
  std::vector<std::string> local_msgs;
  std::vector<std::string>& msgs = msgs_out ? *msgs_out : local_msgs;
  msgs.clear();
  for (size_t j = 0; j < no; ++j) {
    const auto& o = thr.overrides[j];
    std::string perr;
    bool bad = false, begin_ok = false;
    if (!o.begin.empty() && !ParseRFC3339(o.begin, &ob[j], &obn[j], &perr)) {
      bad = true;
      msgs.push_back("index " + std::to_string(j) + ": Failed to parse Begin: " + perr);
    } else if (!o.end.empty() && !ParseRFC3339(o.end, &oe[j], &oen[j], &perr)) {
      bad = begin_ok = true;
      msgs.push_back("index " + std::to_string(j) + ": Failed to parse End: " + perr);
    }
    if (bad) {
      oflags[j] |= KT_OVR_PARSE_ERROR;
      oe[j] = KT_ZERO_TIME_S, oen[j] = 0;
      if (begin_ok) oflags[j] |= KT_OVR_BEGIN_PARSED;  // NextOverrideHappensIn still counts the begin instant
      else ob[j] = KT_ZERO_TIME_S, obn[j] = 0;
    }
    DenseAmount a;
    if (!fill_amount(o.threshold, (int)k, &a, err)) return false;
    std::memcpy(&ov[j * D], a.v, sizeof(int64_t) * D);
    opresent[j] = a.present[0];
    ocount[j] = a.count;
    ohas[j] = a.has_count;
  }
  uint64_t spec_fp = 0;
  for (auto& m : msgs)
    for (char ch : m) spec_fp = (spec_fp ^ (uint8_t)ch) * 1099511628211ull + 0x9E3779B97F4A7C15ull;
  if (!msgs.empty() && spec_fp == 0) spec_fp = 1;
  // selector terms -> requirement pools; LabelSelectorAsSelector validation decides the INVALID flags
  ReqPool preq, nreq;
  const size_t nt = thr.selectorTerms.size();
  std::vector<uint8_t> tflags(nt + 1, 0);
  std::vector<uint32_t> tpo(nt + 1, 0), tno(nt + 1, 0);
  auto convert = [&](const LabelSelector& sel, ReqPool& pool) -> bool {  // returns validity
    bool ok = true;
    for (auto& kv : sel.matchLabels) {
      if (!valid_label_key(kv.first) || !valid_label_value(kv.second)) ok = false;
      pool.add(KT_OP_IN, key_id(kv.first), {pair_id(kv.first, kv.second)});
    }
    for (auto& e : sel.matchExpressions) {
      int op = e.op == "In" ? KT_OP_IN : e.op == "NotIn" ? KT_OP_NOT_IN : e.op == "Exists" ? KT_OP_EXISTS
               : e.op == "DoesNotExist" ? KT_OP_DOES_NOT_EXIST : -1;
      if (op < 0) { ok = false; continue; }
      if ((op == KT_OP_IN || op == KT_OP_NOT_IN) && e.values.empty()) ok = false;
      if ((op == KT_OP_EXISTS || op == KT_OP_DOES_NOT_EXIST) && !e.values.empty()) ok = false;
      if (!valid_label_key(e.key)) ok = false;
      std::vector<uint32_t> vals;
      for (auto& v : e.values) {
        if (!valid_label_value(v)) ok = false;
        vals.push_back(pair_id(e.key, v));
      }
      pool.add((uint8_t)op, key_id(e.key), vals);
    }
    return ok;
  };
  for (size_t j = 0; j < nt; ++j) {
    if (!convert(thr.selectorTerms[j].podSelector, preq)) tflags[j] |= KT_TERM_POD_SEL_INVALID;
    if (thr.cluster && !convert(thr.selectorTerms[j].namespaceSelector, nreq)) tflags[j] |= KT_TERM_NS_SEL_INVALID;
    tpo[j + 1] = (uint32_t)(preq.val_off.size() - 1);
    tno[j + 1] = (uint32_t)(nreq.val_off.size() - 1);
  }
  uint32_t flags = KT_THR_VALID | (thr.cluster ? KT_THR_CLUSTER : 0u);
  if (thr.throttlerName == args.name) flags |= KT_THR_RESPONSIBLE;  // isResponsibleFor (throttle_controller.go:213-215)
  uint32_t zero32 = 0, ooff[2] = {0, (uint32_t)no}, toff[2] = {0, (uint32_t)nt};
  uint64_t zero64 = 0;
  DenseAmount empty;
  kt_snapshot b{};
  b.D = D;
  b.n_thr = 1;
  b.thr_flags = &flags;
  b.thr_ns = &ns32;
  b.thr_spec = kt_amounts{spec.v, &spec.present[0], &spec.count, &spec.has_count};
  b.thr_calc = kt_amounts{empty.v, &empty.present[0], &empty.count, &empty.has_count};
  b.thr_used = b.thr_calc;
  b.thr_reserved = b.thr_calc;
  b.thr_thrl_flag = &zero32;
  b.thr_thrl_has = &zero32;
  b.thr_status_msgs_fp = &zero64;
  b.thr_spec_msgs_fp = &spec_fp;
  b.thr_ovr_off = ooff;
  b.ovr_begin_s = ob.data();
  b.ovr_begin_ns = obn.data();
  b.ovr_end_s = oe.data();
  b.ovr_end_ns = oen.data();
  b.ovr_flags = oflags.data();
  b.ovr_thr = kt_amounts{ov.data(), opresent.data(), ocount.data(), ohas.data()};
  b.thr_term_off = toff;
  b.term_flags = tflags.data();
  b.term_preq_off = tpo.data();
  b.term_nreq_off = tno.data();
  b.preq = preq.view();
  b.nreq = nreq.view();
  int32_t rc = kt_upsert_throttles(pages[k], &b, &r32);
  if (rc != KT_OK) { if (err) *err = engine_error(rc, pages[k]); return false; }
  if (fp_out) *fp_out = spec_fp;
  return true;
}

// Page k is created the first time a resource name fits none of pages 0..k-1.  It is fed what the host's caches hold —
// namespaces, pods, throttles (each with ITS names: none of them names the new page's first name, so they carry nothing
// there yet) and the reserved amounts — and every throttle row that has an applied status gets that status's count part
// (kt_set_status): its own names carry nothing yet, so the page's state is exact.  Rows are kept aligned with page 0,
// the highest throttle row ever used included (kt_paged_* require the same throttle-row count on every page).
bool KubeThrottler::Impl::add_page(std::string* err) {
  if (pages.size() >= (size_t)kMaxPages) {
    if (err) *err = "more than " + std::to_string(D * kMaxPages) + " distinct resource names";
    return false;
  }
  kt_engine* ne = nullptr;
  int32_t rc = kt_engine_create(&cfg, &ne);
  if (rc != KT_OK) {
    if (err) *err = std::string("kt_engine_create: ") + std::to_string(rc) + ": " + kt_last_error(nullptr);
    return false;
  }
  pages.push_back(ne);
  const size_t k = pages.size() - 1;
  for (auto& kv : ns_rows.row_of)
    if (!upsert_namespace(k, kv.first, (int32_t)kv.second, err)) return false;
  for (auto& kv : pod_rows.row_of) {
    auto pit = pods.find(kv.first);
    if (pit == pods.end()) continue;
    if (!upsert_pod(k, pit->second, kv.second, (uint32_t)ns_rows.find(pit->second.ns), err)) return false;
  }
  for (int32_t t = 0; t < (int32_t)thr_rows.next; ++t) {
    if (thr_live[(size_t)t]) {
      const Throttle& thr = thr_by_row[(size_t)t];
      const uint32_t ns32 = thr.cluster ? 0u : (uint32_t)ns_rows.find(thr.ns);
      if (!upsert_throttle(k, thr, t, ns32, nullptr, nullptr, err)) return false;
      const CountPart& c = count_part[(size_t)t];
      if (c.set) {
        DenseAmount used, calc;
        used.count = c.used_count, used.has_count = c.used_has;
        calc.count = c.calc_count, calc.has_count = c.calc_has;
        uint8_t at = c.calc_at_nonzero, pod = c.thrl_pod;
        uint32_t zero = 0;
        uint64_t fp = c.msgs_fp;
        kt_status st{};
        st.used = kt_amounts{used.v, &used.present[0], &used.count, &used.has_count};
        st.calc = kt_amounts{calc.v, &calc.present[0], &calc.count, &calc.has_count};
        st.calc_at_nonzero = &at;
        st.thrl_flag = &zero;
        st.thrl_has = &zero;
        st.thrl_pod = &pod;
        st.msgs_fp = &fp;
        if ((rc = kt_set_status(ne, 1, &t, &st)) != KT_OK) { if (err) *err = engine_error(rc, ne); return false; }
      }
    } else if (t == (int32_t)thr_rows.next - 1) {  // the highest row page 0 ever held is free now: hold it, then free it
      Throttle placeholder;
      if (!upsert_throttle(k, placeholder, t, 0u, nullptr, nullptr, err)) return false;
      if ((rc = kt_delete_throttles(ne, 1, &t)) != KT_OK) { if (err) *err = engine_error(rc, ne); return false; }
    }
  }
  for (auto& kv : reserved)
    if (!push_reserved(kv.first, err, (int)k)) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------
// informer feed
// ---------------------------------------------------------------------------------------------------
bool KubeThrottler::OnNamespaceAdd(const Namespace& ns, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  const int64_t row = p.ns_rows.acquire(ns.name);
  if (row < 0) { if (err) *err = "namespace capacity exhausted"; return false; }
  p.ns_objs[ns.name] = ns;
  for (size_t k = 0; k < p.pages.size(); ++k)
    if (!p.upsert_namespace(k, ns.name, (int32_t)row, err)) return false;
  return true;
}

bool KubeThrottler::OnNamespaceDelete(const std::string& name, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  const int64_t row = p.ns_rows.find(name);
  if (row < 0) return true;
  p.ns_objs.erase(name);
  for (size_t k = 0; k < p.pages.size(); ++k)
    if (!p.upsert_namespace(k, name, (int32_t)row, err)) return false;
  return true;
}

bool KubeThrottler::OnPodAdd(const Pod& pod, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  // every resource name of the pod first: a name that fits no page opens one, fed with what the caches hold so far
  for (auto& ic : pod.initContainers)
    if (!p.register_names(ic.requests, err)) return false;
  for (auto& ct : pod.containers)
    if (!p.register_names(ct.requests, err)) return false;
  if (pod.hasOverhead && !p.register_names(pod.overhead, err)) return false;
  // the pod's namespace id must exist even when no Namespace object was seen (then it stays invalid)
  int64_t ns_row = p.ns_rows.find(pod.ns);
  if (ns_row < 0) {
    ns_row = p.ns_rows.acquire(pod.ns);
    if (ns_row < 0) { if (err) *err = "namespace capacity exhausted"; return false; }
    if (!OnNamespaceDelete(pod.ns, err)) return false;  // registers the id as "no Namespace object"
  }
  if ((int)pod.labels.size() > p.args.maxLabels) { if (err) *err = "pod has more labels than maxLabels"; return false; }
  const int64_t row = p.pod_rows.acquire(pod.Key());
  if (row < 0) { if (err) *err = "pod capacity exhausted"; return false; }
  for (size_t k = 0; k < p.pages.size(); ++k)
    if (!p.upsert_pod(k, pod, row, (uint32_t)ns_row, err)) return false;
  p.pods[pod.Key()] = pod;
  return true;
}

bool KubeThrottler::OnPodDelete(const std::string& key, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  const int64_t row = p.pod_rows.find(key);
  if (row < 0) return true;
  auto known = p.pods.find(key);
  if (known != p.pods.end() && known->second.schedulerName == p.args.targetSchedulerName && !known->second.nodeName.empty())
    Unreserve(known->second);  // "observe the deleted pod is now scheduled. controller should unreserve it."
  for (kt_engine* pe : p.pages) {
    int32_t rc = kt_delete_pods(pe, 1, &row);
    if (rc != KT_OK) { if (err) *err = p.engine_error(rc, pe); return false; }
  }
  p.pod_rows.release(key);
  p.pods.erase(key);
  return true;
}

bool KubeThrottler::OnThrottleAdd(const Throttle& thr, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  if (!p.register_names(thr.threshold, err)) return false;
  for (auto& o : thr.overrides)
    if (!p.register_names(o.threshold, err)) return false;
  int64_t ns_row = 0;
  if (!thr.cluster) {
    ns_row = p.ns_rows.find(thr.ns);
    if (ns_row < 0) {
      ns_row = p.ns_rows.acquire(thr.ns);
      if (ns_row < 0) { if (err) *err = "namespace capacity exhausted"; return false; }
      if (!OnNamespaceDelete(thr.ns, err)) return false;
    }
  }
  const std::string tk = Impl::thr_key(thr);
  const int64_t row = p.thr_rows.acquire(tk);
  if (row < 0) { if (err) *err = "throttle capacity exhausted"; return false; }
  const int32_t r32 = (int32_t)row;
  // The row's stored status starts empty (calculatedAt zero => CheckThrottledFor falls back to spec.threshold,
  // throttle_types.go:129-132) until the next ReconcileAll — the reference enqueues a reconcile for the
  // throttle on the very same Add/Update event (throttle_controller.go:401-417).
  std::vector<std::string> msgs;
  uint64_t fp = 0;
  for (size_t k = 0; k < p.pages.size(); ++k)
    if (!p.upsert_throttle(k, thr, r32, (uint32_t)ns_row, &msgs, &fp, err)) return false;
  p.thr_by_row[(size_t)row] = thr;
  p.thr_live[(size_t)row] = 1;
  p.thr_msgs[(size_t)row] = msgs;
  p.spec_fp[(size_t)row] = fp;
  p.count_part[(size_t)row] = CountPart();
  p.written.erase(tk);
  if (!p.push_reserved(r32, err)) return false;
  return true;
}

bool KubeThrottler::OnThrottleDelete(const std::string& key, bool cluster, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  const std::string tk = (cluster ? "C:" : "T:") + key;
  const int64_t row = p.thr_rows.find(tk);
  if (row < 0) return true;
  const int32_t r32 = (int32_t)row;
  for (kt_engine* pe : p.pages) {
    int32_t rc = kt_delete_throttles(pe, 1, &r32);
    if (rc != KT_OK) { if (err) *err = p.engine_error(rc, pe); return false; }
  }
  p.thr_rows.release(tk);
  p.thr_live[(size_t)row] = 0;
  p.count_part[(size_t)row] = CountPart();
  p.reserved.erase(r32);
  p.written.erase(tk);
  return true;
}

// ---------------------------------------------------------------------------------------------------
// PreFilter / Reserve / Unreserve
// ---------------------------------------------------------------------------------------------------
namespace {
const char* status_name(uint8_t s) {
  switch (s) {
    case KT_STATUS_NOT_THROTTLED: return "not-throttled";
    case KT_STATUS_ACTIVE: return "active";
    case KT_STATUS_INSUFFICIENT: return "insufficient";
    case KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD: return "pod-requests-exceeds-threshold";
    case KT_STATUS_ERROR: return "error";
    default: return "";
  }
}
}  // namespace

// row_always: the caller needs the status row even of an allowed pod (Reserve: which throttles the pod affects)
static bool check_one(KubeThrottler::Impl& p, const Pod& pod, KubeThrottler* self, std::vector<uint8_t>* row_out,
                      uint64_t* summary, std::string* err, bool row_always = true) {
  if (!self->OnPodAdd(pod, err)) return false;  // the engine evaluates what the informer cache would hold
  const int64_t row = p.pod_rows.find(pod.Key());
  int32_t T = 0;
  kt_throttle_rows(p.e, &T);
  row_out->assign((size_t)std::max(T, 1), 0);
  p.last_row_pending = -1;
  if (p.pages.size() > 1) {  // more than one page: the pages combined (kt_paged_check)
    const int32_t rc = kt_paged_check(p.pages.data(), (int32_t)p.pages.size(), 1, &row, /*isThrottledOnEqual=*/0, summary, row_out->data());
    if (rc != KT_OK) {
      if (err) *err = p.engine_error(rc);
      return false;
    }
    row_out->resize((size_t)T);
    return true;
  }
  // the verdict first: one pod, summary word only = the engine's few-pod path (no copy, no stream synchronisation, not
  // queued behind a running reconcile); the status row is only needed to word the reasons of a pod that is not allowed
  int32_t rc = row_always ? KT_OK : kt_check(p.e, 1, &row, /*isThrottledOnEqual=*/0, summary, nullptr);
  p.last_row_pending = -1;
  if (rc == KT_OK && (row_always || *summary != 0))  // blocked or Error: launch + fetch of the row under ONE engine lock
    rc = kt_check(p.e, 1, &row, /*isThrottledOnEqual=*/0, summary, row_out->data());
  else if (rc == KT_OK && row_out == &p.last_status)
    p.last_row_pending = row;
  if (rc != KT_OK) {
    if (err) *err = p.engine_error(rc);
    return false;
  }
  row_out->resize((size_t)T);
  return true;
}

// reasons in the reference's fixed order (plugin.go:182-214)
static std::vector<std::string> block_reasons(const KubeThrottler::Impl& p, const uint8_t* row, size_t n) {
  std::vector<std::string> out;
  static const uint8_t kOrder[] = {KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD, KT_STATUS_ACTIVE, KT_STATUS_INSUFFICIENT};
  for (uint8_t code : kOrder)
    for (int cluster = 1; cluster >= 0; --cluster) {
      std::string names;
      for (size_t t = 0; t < n; ++t) {
        if (!p.thr_live[t] || p.thr_by_row[t].cluster != (cluster == 1) || row[t] != code) continue;
        if (!names.empty()) names += ",";
        names += p.thr_by_row[t].Key();
      }
      if (!names.empty())
        out.push_back(std::string(cluster ? "clusterthrottle[" : "throttle[") + status_name(code) + "]=" + names);
    }
  return out;
}

// the Warning event PreFilter records when the pod's own requests exceed a threshold (plugin.go:190-202):
// ClusterThrottle names first, then Throttle names
static std::vector<Event> block_events(const KubeThrottler::Impl& p, const uint8_t* row, size_t n) {
  std::string names;
  for (int cluster = 1; cluster >= 0; --cluster)
    for (size_t t = 0; t < n; ++t) {
      if (!p.thr_live[t] || p.thr_by_row[t].cluster != (cluster == 1) || row[t] != KT_STATUS_POD_REQUESTS_EXCEEDS_THRESHOLD) continue;
      if (!names.empty()) names += ",";
      names += p.thr_by_row[t].Key();
    }
  if (names.empty()) return {};
  return {Event{"Warning", "ResourceRequestsExceedsThrottleThreshold",
                "It won't be scheduled unless decreasing resource requests or increasing ClusterThrottle/Throttle threshold "
                "because its resource requests exceeds their thresholds: " + names}};
}

Status KubeThrottler::PreFilter(const Pod& pod) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  Status st;
  uint64_t summary = 0;
  std::string err;
  if (!check_one(p, pod, this, &p.last_status, &summary, &err, /*row_always=*/false)) {
    st.code = Error;
    st.reasons.push_back(err);
    return st;
  }
  if (KT_SUMMARY_VERDICT(summary) == KT_VERDICT_ERROR) {  // plugin.go:154-156,166-168
    st.code = Error;
    st.reasons.push_back("throttle check failed for pod " + pod.Key() + " (invalid selector or unknown namespace)");
    return st;
  }
  if (KT_SUMMARY_VERDICT(summary) == KT_VERDICT_SUCCESS) return st;  // plugin.go:177-180
  st.code = UnschedulableAndUnresolvable;
  st.reasons = block_reasons(p, p.last_status.data(), p.last_status.size());
  st.events = block_events(p, p.last_status.data(), p.last_status.size());
  return st;
}

std::string KubeThrottler::LastStatusOf(const std::string& throttle_key) const {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  if (p.last_row_pending >= 0) {  // the last PreFilter allowed the pod on the summary word alone: fetch its row now
    uint64_t summary = 0;
    int64_t row = p.last_row_pending;
    int32_t T = 0;
    kt_throttle_rows(p.e, &T);
    p.last_status.assign((size_t)std::max(T, 1), 0);
    if (kt_check(p.e, 1, &row, 0, &summary, p.last_status.data()) != KT_OK) p.last_status.assign(p.last_status.size(), 0);
    p.last_status.resize((size_t)T);
    p.last_row_pending = -1;
  }
  for (size_t t = 0; t < p.last_status.size(); ++t)
    if (p.thr_live[t] && p.thr_by_row[t].Key() == throttle_key) return status_name(p.last_status[t]);
  return "";
}

Status KubeThrottler::Reserve(const Pod& pod) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  Status st;
  std::vector<uint8_t> row;
  uint64_t summary = 0;
  std::string err;
  if (!check_one(p, pod, this, &row, &summary, &err, /*row_always=*/true) || KT_SUMMARY_VERDICT(summary) == KT_VERDICT_ERROR) {
    st.code = Error;  // plugin.go:223-233
    st.reasons.push_back("Failed to reserve pod=" + pod.Key() + (err.empty() ? "" : ": " + err));
    return st;
  }
  // ResourceAmountOfPod as the engines hold it
  std::vector<DenseAmount> amts;
  const int64_t prow = p.pod_rows.find(pod.Key());
  p.fetch_pod_amounts(1, &prow, &amts);
  const DenseAmount& amt = amts[0];
  for (size_t t = 0; t < row.size(); ++t) {
    if (row[t] == KT_STATUS_NOT_AFFECTED) continue;  // affectedThrottles (throttle_controller.go:271-292)
    p.reserved[(int32_t)t][pod.Key()] = amt;
    if (!p.push_reserved((int32_t)t, &err)) {
      st.code = Error;
      st.reasons.push_back(err);
      return st;
    }
  }
  return st;
}

void KubeThrottler::Unreserve(const Pod& pod) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  for (auto& kv : p.reserved)
    if (kv.second.erase(pod.Key())) p.push_reserved(kv.first, nullptr);
}

bool KubeThrottler::OnPodUpdate(const Pod& old_pod, const Pod& new_pod, std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  auto counts_in = [&](const Pod& q) { return q.schedulerName == p.args.targetSchedulerName && !q.nodeName.empty(); };
  if (old_pod.Key() != new_pod.Key() || (!counts_in(old_pod) && !counts_in(new_pod))) return OnPodAdd(new_pod, err);
  // affectedThrottles(oldPod) and affectedThrottles(newPod): an error on either side skips the move (:459-468)
  std::vector<uint8_t> before, after;
  uint64_t s_before = 0, s_after = 0;
  std::string ignored;
  const bool ok_before = check_one(p, old_pod, this, &before, &s_before, &ignored) && KT_SUMMARY_VERDICT(s_before) != KT_VERDICT_ERROR;
  if (!OnPodAdd(new_pod, err)) return false;  // from here on the engine holds the new object
  const bool ok_after = check_one(p, new_pod, this, &after, &s_after, &ignored) && KT_SUMMARY_VERDICT(s_after) != KT_VERDICT_ERROR;
  if (!ok_before || !ok_after) return true;
  std::vector<DenseAmount> amts;  // ResourceAmountOfPod(newPod), as the engines computed it
  const int64_t prow = p.pod_rows.find(new_pod.Key());
  int32_t rc = p.fetch_pod_amounts(1, &prow, &amts);
  if (rc != KT_OK) { if (err) *err = p.engine_error(rc); return false; }
  const DenseAmount& amt = amts[0];
  const size_t n = std::max(before.size(), after.size());
  for (size_t t = 0; t < n; ++t) {
    const bool was = t < before.size() && before[t] != KT_STATUS_NOT_AFFECTED;
    const bool is = t < after.size() && after[t] != KT_STATUS_NOT_AFFECTED;
    if (was == is) continue;  // common throttles keep whatever they hold (symmetric difference only)
    if (was) {
      auto it = p.reserved.find((int32_t)t);
      if (it == p.reserved.end() || !it->second.erase(new_pod.Key())) continue;
    } else {
      p.reserved[(int32_t)t][new_pod.Key()] = amt;
    }
    if (!p.push_reserved((int32_t)t, err)) return false;
  }
  return true;
}

// One engine launch over the queue positions [i0, i1) (every page: pages[0] == e, usually the only one — the verdicts combined,
// the reservations on every page), committed; the pod-keyed reservation map receives what the engine reserved.  gang_off
// (nullable; [g0, g1] into the queue, gang_off[g0] == i0, gang_off[g1] == i1): the segment in gangs (kt_paged_admit_gangs) — only
// members of ADMITTED gangs enter the map, the engine has already taken the others' amounts out again; admitted[g] receives the flag.
// elastic (nullable, with gang_off): the segment in elastic gangs (kt_paged_admit_gangs_elastic) under min_members [per gang of the
// queue] and required [per queue position, empty: none]; members[g] receives the count, admitted is not used.
struct ElasticRule {
  const std::vector<int64_t>* min_members;
  const std::vector<uint8_t>* required;
  std::vector<int64_t>* members;
};
static void admit_engine_segment(KubeThrottler::Impl& p, const std::vector<std::string>& pod_keys, const std::vector<int64_t>& rows, size_t i0, size_t i1,
                                 std::vector<Status>* out_p, const std::vector<int64_t>* gang_off, std::vector<uint8_t>* admitted, size_t g0 = 0,
                                 size_t g1 = 0, const ElasticRule* elastic = nullptr) {
  std::vector<Status>& out = *out_p;
  const size_t m = i1 - i0;
  if (m == 0) return;
  int32_t T = 0;
  kt_throttle_rows(p.e, &T);
  std::vector<uint64_t> summary(m);
  std::vector<uint8_t> status(m * (size_t)(T > 0 ? T : 1));
  std::vector<DenseAmount> amts;
  std::vector<int64_t> off;      // the segment's gangs, relative to i0
  std::vector<uint8_t> flags;
  int32_t rc;
  std::vector<int64_t> kept;     // elastic: the members that stay, per gang of the segment
  if (gang_off && elastic) {
    for (size_t g = g0; g <= g1; ++g) off.push_back((*gang_off)[g] - (int64_t)i0);
    kept.assign(g1 - g0, 0);
    const bool any_required = !elastic->required->empty();
    rc = kt_paged_admit_gangs_elastic(p.pages.data(), (int32_t)p.pages.size(), (int64_t)m, rows.data() + i0, (int64_t)(g1 - g0), off.data(),
                                      elastic->min_members->data() + g0, any_required ? elastic->required->data() + i0 : nullptr,
                                      /*isThrottledOnEqual=*/0, KT_ADMIT_COMMIT, summary.data(), T > 0 ? status.data() : nullptr, kept.data());
    flags.resize(kept.size());
    for (size_t g = 0; g < kept.size(); ++g) flags[g] = kept[g] > 0 ? 1 : 0;
  } else if (gang_off) {
    for (size_t g = g0; g <= g1; ++g) off.push_back((*gang_off)[g] - (int64_t)i0);
    flags.assign(g1 - g0, 0);
    rc = kt_paged_admit_gangs(p.pages.data(), (int32_t)p.pages.size(), (int64_t)m, rows.data() + i0, (int64_t)(g1 - g0), off.data(),
                              /*isThrottledOnEqual=*/0, KT_ADMIT_COMMIT, summary.data(), T > 0 ? status.data() : nullptr, flags.data());
  } else {
    rc = kt_paged_admit(p.pages.data(), (int32_t)p.pages.size(), (int64_t)m, rows.data() + i0, /*isThrottledOnEqual=*/0, KT_ADMIT_COMMIT,
                        summary.data(), T > 0 ? status.data() : nullptr);
  }
  if (rc == KT_OK) rc = p.fetch_pod_amounts((int64_t)m, rows.data() + i0, &amts);
  if (rc != KT_OK) {
    for (size_t i = i0; i < i1; ++i) out[i].code = Error, out[i].reasons = {p.engine_error(rc)};
    return;
  }
  std::vector<uint8_t> keeps(m, 1);  // the pod's reservation stands (always, without gangs)
  for (size_t g = 0; g + 1 < off.size(); ++g) {
    if (elastic) (*elastic->members)[g0 + g] = kept[g];
    else (*admitted)[g0 + g] = flags[g];
    for (int64_t j = off[g]; j < off[g + 1]; ++j) keeps[(size_t)j] = flags[g];
  }
  for (size_t j = 0; j < m; ++j) {
    const size_t i = i0 + j;
    const uint8_t* row = status.data() + j * (size_t)T;
    const uint64_t v = KT_SUMMARY_VERDICT(summary[j]);
    if (v == KT_VERDICT_ERROR) {
      out[i].code = Error;
      out[i].reasons.push_back("throttle check failed for pod " + pod_keys[i] + " (invalid selector or unknown namespace)");
    } else if (v != KT_VERDICT_SUCCESS) {
      out[i].code = UnschedulableAndUnresolvable;
      out[i].reasons = block_reasons(p, row, (size_t)T);
      out[i].events = block_events(p, row, (size_t)T);
    } else if (keeps[j]) {
      const DenseAmount& amt = amts[j];
      for (int32_t t = 0; t < T; ++t)
        if (row[t] != KT_STATUS_NOT_AFFECTED) p.reserved[t][pod_keys[i]] = amt;  // the engine already holds the totals
    }
  }
}

// One scheduling pass over a queue of pending pods IN ORDER: PreFilter, and on Success Reserve — a single engine
// launch (kt_paged_admit) instead of 2 x n calls.  The reserved cache is updated exactly as n
// Reserve calls would have (reserved_resource_amounts.go:66-77), so Unreserve keeps working pod by pod.
std::vector<Status> KubeThrottler::AdmitQueue(const std::vector<std::string>& pod_keys) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  const size_t n = pod_keys.size();
  std::vector<Status> out(n);
  std::vector<int64_t> rows(n);
  for (size_t i = 0; i < n; ++i) {
    rows[i] = p.pod_rows.find(pod_keys[i]);
    if (rows[i] < 0) {
      for (auto& st : out) st.code = Error, st.reasons = {"pod " + pod_keys[i] + " is not known to the plugin (OnPodAdd first)"};
      return out;
    }
  }
  if (n == 0) return out;
  // The reservation cache is a map keyed by pod (reserved_resource_amounts.go:130-135: c[nn] = amount, idempotent): a pod
  // that is ALREADY reserved somewhere, or named twice in the queue, must not add its amount a second time — neither to
  // the totals nor to what the following pods are checked against.  The engine's queue walk adds every admitted pod, so
  // such a pod ends the current engine segment and goes through the plain PreFilter + Reserve calls; everything else
  // runs as ONE launch per segment (the whole queue in the common case).
  auto already_reserved = [&](const std::string& key) {
    for (auto& kv : p.reserved)
      if (kv.second.count(key)) return true;
    return false;
  };
  auto admit_segment = [&](size_t i0, size_t i1) { admit_engine_segment(p, pod_keys, rows, i0, i1, &out, nullptr, nullptr); };
  size_t seg0 = 0;
  std::set<std::string> in_segment;
  for (size_t i = 0; i < n; ++i) {
    if (!in_segment.count(pod_keys[i]) && !already_reserved(pod_keys[i])) {
      in_segment.insert(pod_keys[i]);
      continue;
    }
    admit_segment(seg0, i);
    const Pod pod = p.pods.at(pod_keys[i]);
    out[i] = PreFilter(pod);
    if (out[i].IsSuccess()) out[i] = Reserve(pod);
    seg0 = i + 1;
    in_segment.clear();
  }
  admit_segment(seg0, n);
  return out;
}

// How many further pods of this pod's shape PreFilter + Reserve would admit in a row, and the throttle that stops the next one:
// kt_paged_headroom over the mirror's pages (the closed form of a dry-run kt_paged_admit of [pod] * cap).  The reserved totals
// are read as they stand — a reservation the pod itself already holds counts like any other — and nothing is changed.
HeadroomResult KubeThrottler::Headroom(const std::string& pod_key, int64_t cap) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  HeadroomResult out;
  const int64_t row = p.pod_rows.find(pod_key);
  if (row < 0) {
    out.error = "pod " + pod_key + " is not known to the plugin (OnPodAdd first)";
    return out;
  }
  int64_t copies = 0;
  int32_t limiting = -1;
  const int32_t rc = kt_paged_headroom(p.pages.data(), (int32_t)p.pages.size(), 1, &row, /*isThrottledOnEqual=*/0, cap, &copies, &limiting);
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    return out;
  }
  out.copies = copies;
  if (limiting >= 0 && (size_t)limiting < p.thr_by_row.size() && p.thr_live[(size_t)limiting]) out.limiting = p.thr_by_row[(size_t)limiting].Key();
  return out;
}

// How many further replicas of this gang AdmitGangs would admit in a row, the throttle that stops the next one and the member it
// stops: one kt_headroom_gangs_launch + kt_headroom_gangs_fetch with the members as ONE gang on the mirror's one engine
// (isThrottledOnEqual = false, as PreFilter).  Nothing is changed.
GangHeadroomResult KubeThrottler::HeadroomGang(const std::vector<std::string>& member_keys, int64_t cap) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  GangHeadroomResult res;
  HeadroomResult& out = res.headroom;
  if (p.pages.size() > 1) {
    out.error = "HeadroomGang: the mirror runs on " + std::to_string(p.pages.size()) + " pages (more than " + std::to_string(p.D) +
                " resource names); the gang headroom has no paged form";
    return res;
  }
  if (member_keys.empty()) {
    out.error = "HeadroomGang: a gang without members";
    return res;
  }
  std::vector<int64_t> rows(member_keys.size());
  std::set<std::string> seen;
  for (size_t i = 0; i < rows.size(); ++i) {
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
    if (!seen.insert(member_keys[i]).second) {  // (it would reserve twice: the engine refuses it too)
      out.error = "HeadroomGang: pod " + member_keys[i] + " is a member twice";
      return res;
    }
  }
  const int64_t gang_off[2] = {0, (int64_t)rows.size()};
  int64_t copies = 0, blocker = -1;
  int32_t limiting = -1;
  int32_t rc = kt_headroom_gangs_launch(p.e, (int64_t)rows.size(), rows.data(), 1, gang_off, /*isThrottledOnEqual=*/0, cap, nullptr);
  if (rc == KT_OK) rc = kt_headroom_gangs_fetch(p.e, 1, &copies, &limiting, &blocker);
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    return res;
  }
  out.copies = copies;
  if (limiting >= 0 && (size_t)limiting < p.thr_by_row.size() && p.thr_live[(size_t)limiting]) out.limiting = p.thr_by_row[(size_t)limiting].Key();
  if (blocker >= 0 && (size_t)blocker < member_keys.size()) res.blocker = member_keys[(size_t)blocker];
  return res;
}

// Which of the candidates have to go before this pod passes PreFilter: kt_preempt_launch + kt_preempt_fetch on the mirror's one
// engine (isThrottledOnEqual = false, as PreFilter).  The reserved totals are read as they stand and nothing is changed.
PreemptResult KubeThrottler::Preempt(const std::string& pod_key, const std::vector<std::string>& candidate_keys,
                                     const std::string& now_rfc3339, bool reprieve) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  PreemptResult out;
  if (p.pages.size() > 1) {
    out.error = "Preempt: the mirror runs on " + std::to_string(p.pages.size()) + " pages (more than " + std::to_string(p.D) +
                " resource names); the preemption query has no paged form";
    return out;
  }
  int64_t now_s;
  int32_t now_ns;
  if (!ParseRFC3339(now_rfc3339, &now_s, &now_ns, &out.error)) return out;
  const int64_t row = p.pod_rows.find(pod_key);
  if (row < 0) {
    out.error = "pod " + pod_key + " is not known to the plugin (OnPodAdd first)";
    return out;
  }
  std::vector<int64_t> cand(candidate_keys.size());
  for (size_t j = 0; j < cand.size(); ++j)
    if ((cand[j] = p.pod_rows.find(candidate_keys[j])) < 0) {
      out.error = "candidate " + candidate_keys[j] + " is not known to the plugin (OnPodAdd first)";
      return out;
    }
  int64_t prefix = KT_PREEMPT_NONE;
  std::vector<uint8_t> mask(cand.size() + 1);
  // with `reprieve` the same launch plus the walk that puts victims back, behind it on the same stream; one fetch either way
  int32_t rc = (reprieve ? kt_preempt_reprieve_launch : kt_preempt_launch)(p.e, 1, &row, (int64_t)cand.size(), cand.data(), now_s, now_ns,
                                                                           /*isThrottledOnEqual=*/0, nullptr);
  if (rc == KT_OK) rc = kt_preempt_fetch(p.e, 1, &prefix, mask.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    return out;
  }
  out.none = prefix < 0;
  for (size_t j = 0; j < cand.size(); ++j)
    if (mask[j]) out.victims.push_back(candidate_keys[j]);
  return out;
}

// Which of the candidates have to go before the whole gang is admitted: kt_preempt_gangs_launch + kt_preempt_gangs_fetch with the
// members as ONE gang on the mirror's one engine (isThrottledOnEqual = false, as PreFilter).  Nothing is changed.
GangPreemptResult KubeThrottler::PreemptGang(const std::vector<std::string>& member_keys, const std::vector<std::string>& candidate_keys,
                                             const std::string& now_rfc3339, bool reprieve) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  GangPreemptResult res;
  PreemptResult& out = res.preempt;
  if (p.pages.size() > 1) {
    out.error = "PreemptGang: the mirror runs on " + std::to_string(p.pages.size()) + " pages (more than " + std::to_string(p.D) +
                " resource names); the preemption query has no paged form";
    return res;
  }
  int64_t now_s;
  int32_t now_ns;
  if (!ParseRFC3339(now_rfc3339, &now_s, &now_ns, &out.error)) return res;
  if (member_keys.empty()) {
    out.error = "PreemptGang: a gang without members";
    return res;
  }
  std::vector<int64_t> rows(member_keys.size()), cand(candidate_keys.size());
  for (size_t i = 0; i < rows.size(); ++i)
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
  for (size_t j = 0; j < cand.size(); ++j)
    if ((cand[j] = p.pod_rows.find(candidate_keys[j])) < 0) {
      out.error = "candidate " + candidate_keys[j] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
  const int64_t gang_off[2] = {0, (int64_t)rows.size()};
  int64_t prefix = KT_PREEMPT_NONE, blocker = -1;
  std::vector<uint8_t> mask(cand.size() + 1);
  // with `reprieve` the same launch plus the walk that puts victims back, behind it on the same stream; one fetch either way
  int32_t rc = (reprieve ? kt_preempt_gangs_reprieve_launch : kt_preempt_gangs_launch)(
      p.e, (int64_t)rows.size(), rows.data(), 1, gang_off, (int64_t)cand.size(), cand.data(), now_s, now_ns, /*isThrottledOnEqual=*/0, nullptr);
  if (rc == KT_OK) rc = kt_preempt_gangs_fetch(p.e, 1, &prefix, mask.data(), &blocker);
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    return res;
  }
  out.none = prefix < 0;
  for (size_t j = 0; j < cand.size(); ++j)
    if (mask[j]) out.victims.push_back(candidate_keys[j]);
  if (blocker >= 0 && (size_t)blocker < member_keys.size()) res.blocker = member_keys[(size_t)blocker];
  return res;
}

// Which of the candidates have to go before the gang's quorum is in: PreemptGang with ElasticGang's rule — one
// kt_preempt_gangs_elastic_launch + kt_preempt_gangs_elastic_fetch with the members as ONE gang on the mirror's one engine
// (isThrottledOnEqual = false, as PreFilter).  Nothing is changed.
ElasticGangPreemptResult KubeThrottler::PreemptElasticGang(const std::vector<std::string>& member_keys, int64_t min_members,
                                                           const std::vector<uint8_t>& required, const std::vector<std::string>& candidate_keys,
                                                           const std::string& now_rfc3339, bool reprieve) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  ElasticGangPreemptResult res;
  PreemptResult& out = res.preempt;
  if (p.pages.size() > 1) {
    out.error = "PreemptElasticGang: the mirror runs on " + std::to_string(p.pages.size()) + " pages (more than " + std::to_string(p.D) +
                " resource names); the preemption query has no paged form";
    return res;
  }
  int64_t now_s;
  int32_t now_ns;
  if (!ParseRFC3339(now_rfc3339, &now_s, &now_ns, &out.error)) return res;
  const size_t size = member_keys.size();
  if (size == 0) {
    out.error = "PreemptElasticGang: a gang without members";
    return res;
  }
  if (min_members < 1 || min_members > (int64_t)size) {  // (worded as AdmitElasticGangs words it)
    out.error = "PreemptElasticGang: gang 0 asks for " + std::to_string(min_members) + " of its " + std::to_string(size) + " members";
    return res;
  }
  if (!required.empty() && required.size() != size) {
    out.error = "PreemptElasticGang: gang 0 has " + std::to_string(size) + " members and " + std::to_string(required.size()) + " required flags";
    return res;
  }
  std::vector<int64_t> rows(size), cand(candidate_keys.size());
  for (size_t i = 0; i < size; ++i)
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
  for (size_t j = 0; j < cand.size(); ++j)
    if ((cand[j] = p.pod_rows.find(candidate_keys[j])) < 0) {
      out.error = "candidate " + candidate_keys[j] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
  std::vector<uint8_t> flags;
  for (size_t i = 0; i < required.size(); ++i) flags.push_back(required[i] ? KT_GANG_MEMBER_REQUIRED : 0);
  const int64_t gang_off[2] = {0, (int64_t)size};
  int64_t prefix = KT_PREEMPT_NONE, blocker = -1;
  std::vector<uint8_t> mask(cand.size() + 1);
  int32_t rc = kt_preempt_gangs_elastic_launch(p.e, (int64_t)size, rows.data(), 1, gang_off, &min_members, flags.empty() ? nullptr : flags.data(),
                                               (int64_t)cand.size(), cand.data(), now_s, now_ns, /*isThrottledOnEqual=*/0,
                                               reprieve ? KT_PREEMPT_REPRIEVE : 0u, nullptr);
  if (rc == KT_OK) rc = kt_preempt_gangs_elastic_fetch(p.e, 1, &prefix, mask.data(), &res.members, &blocker);
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    res.members = 0;
    return res;
  }
  out.none = prefix < 0;
  for (size_t j = 0; j < cand.size(); ++j)
    if (mask[j]) out.victims.push_back(candidate_keys[j]);
  if (blocker >= 0 && (size_t)blocker < size) res.blocker = member_keys[(size_t)blocker];
  return res;
}

// has / instantSec / instantNsec / instant of a RetryAfterResult from the first passing position (KT_FORECAST_NONE: none)
static void retry_after_first(RetryAfterResult& out, int64_t first, const std::vector<int64_t>& inst_s, const std::vector<int32_t>& inst_ns) {
  out.has = first >= 0;
  if (!out.has) return;
  out.instantSec = inst_s[(size_t)first], out.instantNsec = inst_ns[(size_t)first];
  const time_t tt = (time_t)out.instantSec;
  struct tm g;
  gmtime_r(&tt, &g);
  char buf[64];
  size_t n = strftime(buf, sizeof buf, "%Y-%m-%dT%H:%M:%S", &g);
  if (out.instantNsec) n += (size_t)snprintf(buf + n, sizeof buf - n, ".%09d", out.instantNsec);
  snprintf(buf + n, sizeof buf - n, "Z");
  out.instant = buf;
}

// What RetryAfter, RetryAfterGang and their siblings (`who`) share in front of their launch: a mirror on pages refuses, `now` and the horizon are
// checked, then inst = now ++ the override boundaries in (now, now + horizon] (kt_override_instants, twice: count, then fill).
// false: *error says why (an engine error included)
template <class IMPL>
static bool retry_after_instants(IMPL& p, const char* who, const char* query, const std::string& now_rfc3339, int64_t horizon_seconds,
                                 std::vector<int64_t>* inst_s, std::vector<int32_t>* inst_ns, std::string* error) {
  if (p.pages.size() > 1) {
    *error = std::string(who) + ": the mirror runs on " + std::to_string(p.pages.size()) + " pages (more than " + std::to_string(p.D) +
             " resource names); the " + query + " has no paged form";
    return false;
  }
  int64_t now_s;
  int32_t now_ns;
  if (!ParseRFC3339(now_rfc3339, &now_s, &now_ns, error)) return false;
  if (horizon_seconds < 0) {
    *error = std::string(who) + ": horizon " + std::to_string(horizon_seconds) + " s";
    return false;
  }
  int64_t total = 0;
  int32_t rc = kt_override_instants(p.e, now_s, now_ns, now_s + horizon_seconds, now_ns, 0, nullptr, nullptr, &total);
  inst_s->assign((size_t)total + 1, 0), inst_ns->assign((size_t)total + 1, 0);
  (*inst_s)[0] = now_s, (*inst_ns)[0] = now_ns;
  if (rc == KT_OK && total > 0)
    rc = kt_override_instants(p.e, now_s, now_ns, now_s + horizon_seconds, now_ns, total, inst_s->data() + 1, inst_ns->data() + 1, &total);
  if (rc != KT_OK) *error = p.engine_error(rc);
  return rc == KT_OK;
}

// When does this pod pass PreFilter: the override boundaries of the window from the engine's host copy of the specs
// (kt_override_instants: every begin, and end + 1 ns — the first instant an override is no longer active), `now` in front, one
// kt_forecast_launch + kt_forecast_fetch over them on the mirror's one engine (isThrottledOnEqual = false, as PreFilter).
RetryAfterResult KubeThrottler::RetryAfter(const std::string& pod_key, const std::string& now_rfc3339, int64_t horizon_seconds) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  RetryAfterResult out;
  std::vector<int64_t> inst_s;
  std::vector<int32_t> inst_ns;
  if (!retry_after_instants(p, "RetryAfter", "forecast query", now_rfc3339, horizon_seconds, &inst_s, &inst_ns, &out.error)) return out;
  const int64_t row = p.pod_rows.find(pod_key);
  if (row < 0) {
    out.error = "pod " + pod_key + " is not known to the plugin (OnPodAdd first)";
    return out;
  }
  const int64_t m = (int64_t)inst_s.size();
  int64_t first = KT_FORECAST_NONE;
  out.verdicts_at.assign((size_t)m, 0);
  int32_t rc = kt_forecast_launch(p.e, 1, &row, m, inst_s.data(), inst_ns.data(), /*isThrottledOnEqual=*/0, nullptr);
  if (rc == KT_OK) rc = kt_forecast_fetch(p.e, 1, &first, out.verdicts_at.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    out.verdicts_at.clear();
    return out;
  }
  for (int64_t k = 0; k < m; ++k) out.instants.emplace_back(inst_s[(size_t)k], inst_ns[(size_t)k]);
  retry_after_first(out, first, inst_s, inst_ns);
  return out;
}

// When do `want` further pods of this pod's shape fit: RetryAfter's instants, one kt_headroom_forecast_launch +
// kt_headroom_forecast_fetch over them with cap = want on the mirror's one engine (isThrottledOnEqual = false, as PreFilter).
ScaleAfterResult KubeThrottler::ScaleAfter(const std::string& pod_key, int64_t want, const std::string& now_rfc3339, int64_t horizon_seconds) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  ScaleAfterResult out;
  std::vector<int64_t> inst_s;
  std::vector<int32_t> inst_ns;
  if (!retry_after_instants(p, "ScaleAfter", "headroom forecast", now_rfc3339, horizon_seconds, &inst_s, &inst_ns, &out.error)) return out;
  const int64_t row = p.pod_rows.find(pod_key);
  if (row < 0) {
    out.error = "pod " + pod_key + " is not known to the plugin (OnPodAdd first)";
    return out;
  }
  if (want < 1) {
    out.error = "ScaleAfter: want " + std::to_string(want);
    return out;
  }
  const int64_t m = (int64_t)inst_s.size();
  int64_t first = KT_FORECAST_NONE;
  std::vector<int32_t> limiting((size_t)m, -1);
  out.copies_at.assign((size_t)m, 0);
  int32_t rc = kt_headroom_forecast_launch(p.e, 1, &row, m, inst_s.data(), inst_ns.data(), /*isThrottledOnEqual=*/0, /*cap=*/want, want, nullptr);
  if (rc == KT_OK) rc = kt_headroom_forecast_fetch(p.e, 1, &first, out.copies_at.data(), limiting.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    out.copies_at.clear();
    return out;
  }
  for (int64_t k = 0; k < m; ++k) {
    out.instants.emplace_back(inst_s[(size_t)k], inst_ns[(size_t)k]);
    const int32_t t = limiting[(size_t)k];
    out.limiting_at.push_back(t >= 0 && (size_t)t < p.thr_by_row.size() && p.thr_live[(size_t)t] ? p.thr_by_row[(size_t)t].Key() : std::string());
  }
  RetryAfterResult at;  // (the instant's text is RetryAfter's)
  retry_after_first(at, first, inst_s, inst_ns);
  out.found = at.has, out.instantSec = at.instantSec, out.instantNsec = at.instantNsec, out.instant = at.instant;
  return out;
}

// When is this gang admitted: RetryAfter's instants, one kt_forecast_gangs_launch + kt_forecast_gangs_fetch with the members as ONE
// gang on the mirror's one engine (isThrottledOnEqual = false, as PreFilter).  Nothing is changed.
GangRetryAfterResult KubeThrottler::RetryAfterGang(const std::vector<std::string>& member_keys, const std::string& now_rfc3339,
                                                   int64_t horizon_seconds) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  GangRetryAfterResult res;
  RetryAfterResult& out = res.retry;
  std::vector<int64_t> inst_s;
  std::vector<int32_t> inst_ns;
  if (!retry_after_instants(p, "RetryAfterGang", "gang forecast", now_rfc3339, horizon_seconds, &inst_s, &inst_ns, &out.error)) return res;
  if (member_keys.empty()) {
    out.error = "RetryAfterGang: a gang without members";
    return res;
  }
  std::vector<int64_t> rows(member_keys.size());
  std::set<std::string> seen;
  for (size_t i = 0; i < rows.size(); ++i) {
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
    if (!seen.insert(member_keys[i]).second) {  // (it would reserve twice: the engine refuses it too)
      out.error = "RetryAfterGang: pod " + member_keys[i] + " is a member twice";
      return res;
    }
  }
  const int64_t m = (int64_t)inst_s.size();
  const int64_t gang_off[2] = {0, (int64_t)rows.size()};
  int64_t first = KT_FORECAST_NONE;
  std::vector<int64_t> blockers((size_t)m, -1);
  out.verdicts_at.assign((size_t)m, 0);
  int32_t rc = kt_forecast_gangs_launch(p.e, (int64_t)rows.size(), rows.data(), 1, gang_off, m, inst_s.data(), inst_ns.data(),
                                        /*isThrottledOnEqual=*/0, nullptr);
  if (rc == KT_OK) rc = kt_forecast_gangs_fetch(p.e, 1, &first, out.verdicts_at.data(), blockers.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    out.verdicts_at.clear();
    return res;
  }
  for (int64_t k = 0; k < m; ++k) {
    out.instants.emplace_back(inst_s[(size_t)k], inst_ns[(size_t)k]);
    const int64_t b = blockers[(size_t)k];
    res.blockers_at.push_back(b >= 0 && (size_t)b < member_keys.size() ? member_keys[(size_t)b] : std::string());
  }
  retry_after_first(out, first, inst_s, inst_ns);
  return res;
}

// When does this gang's quorum fit: RetryAfterGang with ElasticGang's rule — RetryAfter's instants, one
// kt_forecast_gangs_elastic_launch + kt_forecast_gangs_elastic_fetch with the members as ONE gang on the mirror's one engine
// (isThrottledOnEqual = false, as PreFilter).  Nothing is changed.
ElasticGangRetryAfterResult KubeThrottler::RetryAfterElasticGang(const std::vector<std::string>& member_keys, int64_t min_members,
                                                                 const std::vector<uint8_t>& required, const std::string& now_rfc3339,
                                                                 int64_t horizon_seconds) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  ElasticGangRetryAfterResult res;
  RetryAfterResult& out = res.retry;
  std::vector<int64_t> inst_s;
  std::vector<int32_t> inst_ns;
  if (!retry_after_instants(p, "RetryAfterElasticGang", "elastic gang forecast", now_rfc3339, horizon_seconds, &inst_s, &inst_ns, &out.error))
    return res;
  const size_t size = member_keys.size();
  if (size == 0) {
    out.error = "RetryAfterElasticGang: a gang without members";
    return res;
  }
  if (min_members < 1 || min_members > (int64_t)size) {  // (worded as AdmitElasticGangs words it)
    out.error = "RetryAfterElasticGang: gang 0 asks for " + std::to_string(min_members) + " of its " + std::to_string(size) + " members";
    return res;
  }
  if (!required.empty() && required.size() != size) {
    out.error = "RetryAfterElasticGang: gang 0 has " + std::to_string(size) + " members and " + std::to_string(required.size()) + " required flags";
    return res;
  }
  std::vector<int64_t> rows(size);
  std::set<std::string> seen;
  for (size_t i = 0; i < size; ++i) {
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
    if (!seen.insert(member_keys[i]).second) {  // (it would reserve twice: the engine refuses it too)
      out.error = "RetryAfterElasticGang: pod " + member_keys[i] + " is a member twice";
      return res;
    }
  }
  std::vector<uint8_t> flags;
  for (size_t i = 0; i < required.size(); ++i) flags.push_back(required[i] ? KT_GANG_MEMBER_REQUIRED : 0);
  const int64_t m = (int64_t)inst_s.size();
  const int64_t gang_off[2] = {0, (int64_t)size};
  int64_t first = KT_FORECAST_NONE;
  std::vector<int64_t> blockers((size_t)m, -1);
  out.verdicts_at.assign((size_t)m, 0);
  res.members_at.assign((size_t)m, 0);
  int32_t rc = kt_forecast_gangs_elastic_launch(p.e, (int64_t)size, rows.data(), 1, gang_off, &min_members, flags.empty() ? nullptr : flags.data(), m,
                                                inst_s.data(), inst_ns.data(), /*isThrottledOnEqual=*/0, nullptr);
  if (rc == KT_OK) rc = kt_forecast_gangs_elastic_fetch(p.e, 1, &first, out.verdicts_at.data(), res.members_at.data(), blockers.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    out.verdicts_at.clear();
    res.members_at.clear();
    return res;
  }
  for (int64_t k = 0; k < m; ++k) {
    out.instants.emplace_back(inst_s[(size_t)k], inst_ns[(size_t)k]);
    const int64_t b = blockers[(size_t)k];
    res.blockers_at.push_back(b >= 0 && (size_t)b < size ? member_keys[(size_t)b] : std::string());
  }
  retry_after_first(out, first, inst_s, inst_ns);
  return res;
}

// When do `want` further replicas of this gang fit: RetryAfter's instants, one kt_headroom_forecast_gangs_launch +
// kt_headroom_forecast_gangs_fetch with the members as ONE gang and cap = want on the mirror's one engine (isThrottledOnEqual =
// false, as PreFilter).  Nothing is changed.
GangScaleAfterResult KubeThrottler::ScaleAfterGang(const std::vector<std::string>& member_keys, int64_t want, const std::string& now_rfc3339,
                                                   int64_t horizon_seconds) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  GangScaleAfterResult res;
  ScaleAfterResult& out = res.scale;
  std::vector<int64_t> inst_s;
  std::vector<int32_t> inst_ns;
  if (!retry_after_instants(p, "ScaleAfterGang", "gang headroom forecast", now_rfc3339, horizon_seconds, &inst_s, &inst_ns, &out.error)) return res;
  if (member_keys.empty()) {
    out.error = "ScaleAfterGang: a gang without members";
    return res;
  }
  std::vector<int64_t> rows(member_keys.size());
  std::set<std::string> seen;
  for (size_t i = 0; i < rows.size(); ++i) {
    if ((rows[i] = p.pod_rows.find(member_keys[i])) < 0) {
      out.error = "pod " + member_keys[i] + " is not known to the plugin (OnPodAdd first)";
      return res;
    }
    if (!seen.insert(member_keys[i]).second) {  // (it would reserve twice: the engine refuses it too)
      out.error = "ScaleAfterGang: pod " + member_keys[i] + " is a member twice";
      return res;
    }
  }
  if (want < 1) {
    out.error = "ScaleAfterGang: want " + std::to_string(want);
    return res;
  }
  const int64_t m = (int64_t)inst_s.size();
  const int64_t gang_off[2] = {0, (int64_t)rows.size()};
  int64_t first = KT_FORECAST_NONE;
  std::vector<int32_t> limiting((size_t)m, -1);
  std::vector<int64_t> blockers((size_t)m, -1);
  out.copies_at.assign((size_t)m, 0);
  int32_t rc = kt_headroom_forecast_gangs_launch(p.e, (int64_t)rows.size(), rows.data(), 1, gang_off, m, inst_s.data(), inst_ns.data(),
                                                 /*isThrottledOnEqual=*/0, /*cap=*/want, want, nullptr);
  if (rc == KT_OK) rc = kt_headroom_forecast_gangs_fetch(p.e, 1, &first, out.copies_at.data(), limiting.data(), blockers.data());
  if (rc != KT_OK) {
    out.error = p.engine_error(rc);
    out.copies_at.clear();
    return res;
  }
  for (int64_t k = 0; k < m; ++k) {
    out.instants.emplace_back(inst_s[(size_t)k], inst_ns[(size_t)k]);
    const int32_t t = limiting[(size_t)k];
    out.limiting_at.push_back(t >= 0 && (size_t)t < p.thr_by_row.size() && p.thr_live[(size_t)t] ? p.thr_by_row[(size_t)t].Key() : std::string());
    const int64_t b = blockers[(size_t)k];
    res.blockers_at.push_back(b >= 0 && (size_t)b < member_keys.size() ? member_keys[(size_t)b] : std::string());
  }
  RetryAfterResult at;  // (the instant's text is RetryAfter's)
  retry_after_first(at, first, inst_s, inst_ns);
  out.found = at.has, out.instantSec = at.instantSec, out.instantNsec = at.instantNsec, out.instant = at.instant;
  return res;
}

// A scheduling pass over a queue of GANGS (jobs whose pods only run together), in order: every member gets PreFilter and, on
// Success, Reserve; a gang with a member that did not succeed gets Unreserve for all its members (plugin.go:240-257) before the next
// gang is looked at — ONE engine launch per segment (kt_paged_admit_gangs) instead of up to 3 x n calls.  Segments end on gang
// boundaries; a gang that holds a pod which is already reserved, or one named twice (in the gang or earlier in the segment), goes the
// plain way — the engine's walk would add that pod's amount a second time (see AdmitQueue).
GangAdmission KubeThrottler::AdmitGangs(const std::vector<std::vector<std::string>>& gangs) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  GangAdmission res;
  std::vector<std::string> pod_keys;
  std::vector<int64_t> gang_off{0};
  for (auto& g : gangs) {
    pod_keys.insert(pod_keys.end(), g.begin(), g.end());
    gang_off.push_back((int64_t)pod_keys.size());
  }
  const size_t n = pod_keys.size(), G = gangs.size();
  res.status.assign(n, Status{});
  res.admitted.assign(G, 0);
  std::vector<int64_t> rows(n);
  for (size_t i = 0; i < n; ++i) {
    rows[i] = p.pod_rows.find(pod_keys[i]);
    if (rows[i] < 0) {
      for (auto& st : res.status) st.code = Error, st.reasons = {"pod " + pod_keys[i] + " is not known to the plugin (OnPodAdd first)"};
      return res;
    }
  }
  auto already_reserved = [&](const std::string& key) {
    for (auto& kv : p.reserved)
      if (kv.second.count(key)) return true;
    return false;
  };
  size_t seg0 = 0;  // first gang of the current engine segment
  std::set<std::string> in_segment;
  auto flush = [&](size_t g_end) {
    if (g_end > seg0)
      admit_engine_segment(p, pod_keys, rows, (size_t)gang_off[seg0], (size_t)gang_off[g_end], &res.status, &gang_off, &res.admitted, seg0, g_end);
    in_segment.clear();
  };
  for (size_t g = 0; g < G; ++g) {
    if (gangs[g].empty()) {  // nothing to place: admitted, and no engine gang (the C-ABI refuses empty ones)
      flush(g);
      res.admitted[g] = 1;
      seg0 = g + 1;
      continue;
    }
    bool plain = false;
    std::set<std::string> own;
    for (auto& key : gangs[g]) plain |= !own.insert(key).second || in_segment.count(key) || already_reserved(key);
    if (!plain) {
      in_segment.insert(own.begin(), own.end());
      continue;
    }
    flush(g);
    bool all = true;
    for (int64_t i = gang_off[g]; i < gang_off[g + 1]; ++i) {
      const Pod pod = p.pods.at(pod_keys[(size_t)i]);
      Status& st = res.status[(size_t)i];
      st = PreFilter(pod);
      if (st.IsSuccess()) st = Reserve(pod);
      all &= st.IsSuccess();
    }
    if (!all)
      for (int64_t i = gang_off[g]; i < gang_off[g + 1]; ++i) Unreserve(p.pods.at(pod_keys[(size_t)i]));
    res.admitted[g] = all ? 1 : 0;
    seg0 = g + 1;
  }
  flush(G);
  return res;
}

// The same pass over ELASTIC gangs (a job that starts once its quorum of pods fits, PodGroup.minMember / minAvailable, with
// members that can be made mandatory): ONE engine launch per segment (kt_paged_admit_gangs_elastic), the segments of AdmitGangs.  A gang
// that goes the plain way: PreFilter per member and Reserve on Success, then Unreserve of all members if the rule fails.
ElasticGangAdmission KubeThrottler::AdmitElasticGangs(const std::vector<ElasticGang>& gangs) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  ElasticGangAdmission res;
  std::vector<std::string> pod_keys;
  std::vector<int64_t> gang_off{0}, min_members;
  std::vector<uint8_t> required;
  bool any_required = false;
  for (auto& g : gangs) {
    pod_keys.insert(pod_keys.end(), g.members.begin(), g.members.end());
    gang_off.push_back((int64_t)pod_keys.size());
    min_members.push_back(g.min_members);
    any_required |= !g.required.empty();
  }
  const size_t n = pod_keys.size(), G = gangs.size();
  res.status.assign(n, Status{});
  res.members.assign(G, 0);
  auto refuse = [&](const std::string& why) {
    for (auto& st : res.status) st.code = Error, st.reasons = {why};
    return res;
  };
  for (size_t g = 0; g < G; ++g) {
    const size_t size = gangs[g].members.size();
    if (size && (gangs[g].min_members < 1 || gangs[g].min_members > (int64_t)size))
      return refuse("AdmitElasticGangs: gang " + std::to_string(g) + " asks for " + std::to_string(gangs[g].min_members) + " of its " +
                    std::to_string(size) + " members");
    if (!gangs[g].required.empty() && gangs[g].required.size() != size)
      return refuse("AdmitElasticGangs: gang " + std::to_string(g) + " has " + std::to_string(size) + " members and " +
                    std::to_string(gangs[g].required.size()) + " required flags");
    if (any_required)
      for (size_t j = 0; j < size; ++j) required.push_back(!gangs[g].required.empty() && gangs[g].required[j] ? KT_GANG_MEMBER_REQUIRED : 0);
  }
  std::vector<int64_t> rows(n);
  for (size_t i = 0; i < n; ++i) {
    rows[i] = p.pod_rows.find(pod_keys[i]);
    if (rows[i] < 0) return refuse("pod " + pod_keys[i] + " is not known to the plugin (OnPodAdd first)");
  }
  auto already_reserved = [&](const std::string& key) {
    for (auto& kv : p.reserved)
      if (kv.second.count(key)) return true;
    return false;
  };
  const ElasticRule rule{&min_members, &required, &res.members};
  size_t seg0 = 0;  // first gang of the current engine segment
  std::set<std::string> in_segment;
  auto flush = [&](size_t g_end) {
    if (g_end > seg0)
      admit_engine_segment(p, pod_keys, rows, (size_t)gang_off[seg0], (size_t)gang_off[g_end], &res.status, &gang_off, nullptr, seg0, g_end, &rule);
    in_segment.clear();
  };
  for (size_t g = 0; g < G; ++g) {
    if (gangs[g].members.empty()) {  // nothing to place: admitted with no members, and no engine gang (the C-ABI refuses empty ones)
      flush(g);
      seg0 = g + 1;
      continue;
    }
    bool plain = false;
    std::set<std::string> own;
    for (auto& key : gangs[g].members) plain |= !own.insert(key).second || in_segment.count(key) || already_reserved(key);
    if (!plain) {
      in_segment.insert(own.begin(), own.end());
      continue;
    }
    flush(g);
    int64_t n_in = 0;
    bool required_out = false;
    for (int64_t i = gang_off[g]; i < gang_off[g + 1]; ++i) {
      const Pod pod = p.pods.at(pod_keys[(size_t)i]);
      Status& st = res.status[(size_t)i];
      st = PreFilter(pod);
      if (st.IsSuccess()) st = Reserve(pod);
      if (st.IsSuccess()) ++n_in;
      else if (any_required && required[(size_t)i]) required_out = true;
    }
    const bool kept = n_in >= gangs[g].min_members && !required_out;
    if (!kept)
      for (int64_t i = gang_off[g]; i < gang_off[g + 1]; ++i) Unreserve(p.pods.at(pod_keys[(size_t)i]));
    res.members[g] = kept ? n_in : 0;
    seg0 = g + 1;
  }
  flush(G);
  return res;
}

// ---------------------------------------------------------------------------------------------------
// reconcile
// ---------------------------------------------------------------------------------------------------
bool KubeThrottler::ReconcileAll(const std::string& now_rfc3339, std::map<std::string, ThrottleStatus>* out,
                                 std::string* err) {
  std::lock_guard<std::recursive_mutex> lk(p_->mu);
  auto& p = *p_;
  int64_t now_s;
  int32_t now_ns;
  if (!ParseRFC3339(now_rfc3339, &now_s, &now_ns, err)) return false;
  int32_t T = 0;
  kt_throttle_rows(p.e, &T);
  const int D = p.D;
  const size_t N = (size_t)std::max(T, 1);
  std::vector<int64_t> uv(N * D), ucount(N), cv(N * D), ccount(N);
  std::vector<uint32_t> upresent(N), cpresent(N), tflag(N), thas(N);
  std::vector<uint8_t> uhas(N), chas(N), updated(N), tpod(N), terr(N);
  kt_status st{};
  st.used = kt_amounts{uv.data(), upresent.data(), ucount.data(), uhas.data()};
  st.calc = kt_amounts{cv.data(), cpresent.data(), ccount.data(), chas.data()};
  st.calc_at_nonzero = updated.data();
  st.thrl_flag = tflag.data();
  st.thrl_has = thas.data();
  st.thrl_pod = tpod.data();
  st.error = terr.data();
  // pages 1..: their own names' used / throttled (page_out[k]); the count part, the flags and the next override are page 0's
  const size_t NP = p.pages.size();
  std::vector<std::vector<int64_t>> puv(NP), pucount(NP), pcv(NP), pccount(NP);
  std::vector<std::vector<uint32_t>> pupresent(NP), pcpresent(NP), ptflag(NP), pthas(NP);
  std::vector<std::vector<uint8_t>> puhas(NP), pchas(NP), pupdated(NP), ptpod(NP), pterr(NP);
  std::vector<kt_status> page_out(NP, st);
  for (size_t k = 1; k < NP; ++k) {
    puv[k].resize(N * D), pucount[k].resize(N), pcv[k].resize(N * D), pccount[k].resize(N);
    pupresent[k].resize(N), pcpresent[k].resize(N), ptflag[k].resize(N), pthas[k].resize(N);
    puhas[k].resize(N), pchas[k].resize(N), pupdated[k].resize(N), ptpod[k].resize(N), pterr[k].resize(N);
    kt_status& o = page_out[k];
    o.used = kt_amounts{puv[k].data(), pupresent[k].data(), pucount[k].data(), puhas[k].data()};
    o.calc = kt_amounts{pcv[k].data(), pcpresent[k].data(), pccount[k].data(), pchas[k].data()};
    o.calc_at_nonzero = pupdated[k].data();
    o.thrl_flag = ptflag[k].data();
    o.thrl_has = pthas[k].data();
    o.thrl_pod = ptpod[k].data();
    o.error = pterr[k].data();
  }
  std::vector<uint8_t> updated0(N);  // page 0's own "replaced" flag: what ITS stored calculatedAt follows
  int32_t rc;
  if (NP == 1) {
    rc = kt_reconcile_launch(p.e, now_s, now_ns, KT_RECONCILE_APPLY, nullptr);
    if (rc == KT_OK) rc = kt_reconcile_fetch(p.e, T, &st);
    updated0 = updated;
  } else {
    std::vector<uint8_t> replaced_any(N), error_any(N);
    rc = kt_paged_reconcile(p.pages.data(), (int32_t)NP, now_s, now_ns, KT_RECONCILE_APPLY, T, page_out.data(), replaced_any.data(), error_any.data());
    updated0 = updated;
    for (size_t t = 0; t < N; ++t) updated[t] = replaced_any[t], terr[t] = error_any[t];
  }
  std::vector<int64_t> nx_s((size_t)T + 1);
  std::vector<int32_t> nx_ns((size_t)T + 1);
  std::vector<uint8_t> nx_has((size_t)T + 1);
  if (rc == KT_OK) rc = kt_reconcile_fetch_next_override(p.e, T, nx_s.data(), nx_ns.data(), nx_has.data());
  if (rc != KT_OK) {
    if (err) *err = p.engine_error(rc);
    return false;
  }
  // Once status is updated, the reconciled throttle's AFFECTED pods are safe to un-reserve (unreserveAffectedPods,
  // throttle_controller.go:135-155 / clusterthrottle_controller.go:138-160: it walks affectedNonTerminatedPods +
  // affectedTerminatedPods of the throttle — shouldCountIn AND the selector matches the pod as it is now).  A pod that was
  // reserved on the throttle and whose labels moved on afterwards is NOT in that list: its reservation stays until the pod
  // handlers move it (kt_affected_pods: one small check launch over the pods that hold reservations).
  {
    std::vector<int32_t> thr_list;   // reconciled throttles that hold reservations
    std::vector<std::string> keys;   // counted pods that hold a reservation on one of them
    std::map<std::string, size_t> key_ix;
    for (auto& kv : p.reserved) {
      // a reconcile that failed returned before unreserveAffectedPods (throttle_controller.go:103-106), and throttles of
      // another throttler are never reconciled: their reservations stay
      const int32_t t = kv.first;
      if (t < 0 || t >= T || terr[(size_t)t] || !p.thr_live[(size_t)t] || p.thr_by_row[(size_t)t].throttlerName != p.args.name) continue;
      bool any = false;
      for (auto& r : kv.second) {
        auto pit = p.pods.find(r.first);
        const bool counted = pit != p.pods.end() && pit->second.schedulerName == p.args.targetSchedulerName && !pit->second.nodeName.empty();
        if (!counted || p.pod_rows.find(r.first) < 0) continue;
        if (!key_ix.count(r.first)) key_ix[r.first] = keys.size(), keys.push_back(r.first);
        any = true;
      }
      if (any) thr_list.push_back(t);
    }
    if (!keys.empty() && !thr_list.empty()) {
      std::vector<int64_t> rows(keys.size());
      for (size_t i = 0; i < keys.size(); ++i) rows[i] = p.pod_rows.find(keys[i]);
      std::vector<uint8_t> aff(keys.size() * thr_list.size());
      rc = kt_affected_pods(p.e, (int64_t)rows.size(), rows.data(), (int32_t)thr_list.size(), thr_list.data(), aff.data());
      if (rc != KT_OK) {
        if (err) *err = p.engine_error(rc);
        return false;
      }
      for (size_t j = 0; j < thr_list.size(); ++j) {
        auto& held = p.reserved[thr_list[j]];
        bool changed = false;
        for (auto it = held.begin(); it != held.end();) {
          auto k = key_ix.find(it->first);
          if (k != key_ix.end() && aff[k->second * thr_list.size() + j] == 1) it = held.erase(it), changed = true;
          else ++it;
        }
        if (changed) p.push_reserved(thr_list[j], nullptr);
      }
    }
  }
  // the count part of every applied status, kept for a page that is created later (Impl::add_page); page 0's calculatedAt
  // becomes non-zero when page 0's calculatedThreshold is replaced, its messages then are the spec's
  for (int32_t t = 0; t < T; ++t) {
    if (!p.thr_live[(size_t)t] || p.thr_by_row[(size_t)t].throttlerName != p.args.name || terr[(size_t)t]) continue;
    CountPart& c = p.count_part[(size_t)t];
    c.set = true;
    c.used_count = ucount[(size_t)t], c.used_has = uhas[(size_t)t];
    c.calc_count = ccount[(size_t)t], c.calc_has = chas[(size_t)t];
    c.thrl_pod = tpod[(size_t)t];
    if (updated0[(size_t)t]) c.calc_at_nonzero = 1, c.msgs_fp = p.spec_fp[(size_t)t];
  }
  const size_t n_names = (size_t)D * NP;
  std::vector<std::string> dim_name(n_names);
  std::vector<int> dim_scale(n_names, 0);
  for (auto& kv : p.dims) {
    const size_t g = (size_t)kv.second.page * (size_t)D + (size_t)kv.second.dim;
    dim_name[g] = kv.first, dim_scale[g] = kv.second.scale;
  }
  for (int32_t t = 0; t < T; ++t) {
    if (!p.thr_live[(size_t)t] || p.thr_by_row[(size_t)t].throttlerName != p.args.name) continue;
    ThrottleStatus s;
    s.error = terr[t] != 0;
    s.usedHasCounts = uhas[t] != 0;
    s.usedPod = ucount[t];
    s.throttledPod = tpod[t] != 0;
    s.calculatedThresholdUpdated = updated[t] != 0;
    s.messages = p.thr_msgs[(size_t)t];
    s.hasNextOverride = nx_has[(size_t)t] != 0;  // NextOverrideHappensIn -> enqueueAfter (throttle_controller.go:201-208)
    s.nextOverrideSec = nx_s[(size_t)t];
    s.nextOverrideNsec = nx_ns[(size_t)t];
    for (size_t pg = 0; pg < NP; ++pg) {  // each name from the page that owns it
      const uint32_t up = pg ? pupresent[pg][(size_t)t] : upresent[t];
      const int64_t* uvp = pg ? puv[pg].data() : uv.data();
      const uint32_t th = pg ? pthas[pg][(size_t)t] : thas[t], tf = pg ? ptflag[pg][(size_t)t] : tflag[t];
      for (int d = 0; d < D; ++d) {
        const size_t g = pg * (size_t)D + (size_t)d;
        if ((up >> d) & 1u) {
          Quantity q;
          q.nano = (__int128)uvp[(size_t)t * D + d];
          for (int k = 0; k < 9 + dim_scale[g]; ++k) q.nano *= 10;
          auto f = p.dim_format.find(dim_name[g]);
          if (f != p.dim_format.end()) q.format = f->second;
          s.used[dim_name[g]] = q;
        }
        if ((th >> d) & 1u) s.throttledRequests[dim_name[g]] = (tf >> d) & 1u;
      }
    }
    if (!s.error) {  // a reconcile error returns before any status is built (throttle_controller.go:103-106)
      ThrottleStatus& prev = p.written[Impl::thr_key(p.thr_by_row[(size_t)t])];
      s.needsUpdate = s.calculatedThresholdUpdated || !StatusSemanticEqual(prev, s);
      prev = s;
    }
    if (out) (*out)[p.thr_by_row[(size_t)t].Key()] = s;
  }
  return true;
}

}  // namespace kth
