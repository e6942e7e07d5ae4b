// Test of the C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with a PickerKind::Bounded profile that has flow_weights and a
// turn_window (SEMANTICS.md §3h).  Without an argument (no device needed): Configure refuses weights or a window without n_flows, a
// weight array of the wrong size and a zero weight, by profile name.  With `gpu`: a `decode` profile with two bands, three flows of
// weights (3, 1, 1) and no window, whose results must equal direct eppk_pick_wfair calls on the same rows (a context of its own with the
// same chain and snapshot), pick for pick, and differ from eppk_pick_fair (the weights decide); then the same profile with a window,
// the same batch three times: every batch equals a direct call fed with the turns of the one before and rebased as the scheduler
// rebases, the scheduler's table equals the direct one, and the second batch does not place the requests the first placed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gateway-api-inference-extension_amd/host/eppk_host.hpp"

using namespace eppk_host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// every request runs the one profile
class OneProfile : public ProfileHandler {
 public:
  std::vector<std::string> Pick(const Request&, const std::vector<std::string>& profiles, const std::map<std::string, std::vector<ScoredEndpoint>>& done) override {
    return done.empty() ? profiles : std::vector<std::string>{};
  }
  SchedulingResult ProcessResults(const Request&, const std::map<std::string, std::vector<ScoredEndpoint>>& results) override {
    SchedulingResult out;
    for (const auto& kv : results) {
      auto& v = out.profile_results[kv.first];
      for (const ScoredEndpoint& e : kv.second) v.push_back(e.endpoint);
    }
    out.primary_profile_name = "decode";
    return out;
  }
};

static void MakeRows(const std::vector<Request>& reqs, const std::string& model, int B, std::vector<uint8_t>* rb) {
  const size_t stride = 8u + 8u * (size_t)B;
  rb->assign(reqs.size() * stride, 0);
  for (size_t i = 0; i < reqs.size(); ++i) {
    const Request& rq = reqs[i];
    eppk_req_hdr hdr; hdr.adapter = -1;
    hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)rq.prompt.data(), rq.prompt.size(), 64,
                                              (uint64_t*)(rb->data() + i * stride + 8), (uint32_t)B);
    std::memcpy(rb->data() + i * stride, &hdr, 8);
  }
}

// the scheduler's answers for a batch against picks of a direct call
static bool SamePicks(const std::vector<SchedulingResult>& res, const std::vector<Status>& st, const std::vector<int32_t>& picks, const std::vector<Endpoint>& eps) {
  for (size_t i = 0; i < picks.size(); ++i) {
    auto it = res[i].profile_results.find("decode");
    if (it == res[i].profile_results.end()) return false;
    if (picks[i] < 0 ? !(it->second.empty() && st[i].code == Code::Unavailable)
                     : !(it->second.size() == 1 && it->second[0]->address == eps[(size_t)picks[i]].address && st[i].ok())) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  const int P = 6, B = 8;
  const uint32_t kFlows = 3;
  const std::vector<uint16_t> weights{3, 1, 1};
  std::vector<ProfileSpec> specs(1);
  specs[0].name = "decode";
  specs[0].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_KV, 5}};
  specs[0].picker = PickerKind::Bounded;
  specs[0].k = 2;
  specs[0].cap_all = 5;
  specs[0].n_flows = kFlows;
  specs[0].flow_weights = weights;
  specs[0].bands = {{EPPK_BOUNDED_SHED, 0}, {EPPK_BOUNDED_SHED, 2}};
  OneProfile handler;
  Scheduler::Options opt;
  opt.max_pods = 64; opt.max_blocks = B; opt.max_batch = 128;
  opt.index_slots = 1024;
  {                                                                                // refused before any context is created
    auto refused = [&](const ProfileSpec& ps, const char* word) {
      Scheduler s;
      const Status rs = s.Configure({ps}, &handler, opt);
      return !rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find(word) != std::string::npos;
    };
    ProfileSpec bad = specs[0];
    bad.n_flows = 0;
    CHECK(refused(bad, "need n_flows"));                                           // weights without flows
    bad.flow_weights.clear();
    bad.turn_window = 3;
    CHECK(refused(bad, "need n_flows"));                                           // a window without flows
    bad = specs[0];
    bad.flow_weights = {3, 1};
    CHECK(refused(bad, "2 entries for 3 flows"));
    bad.flow_weights = {3, 0, 1};
    CHECK(refused(bad, "flow_weights[1] is 0"));
    CHECK(ProfileSpec{}.flow_weights.empty() && ProfileSpec{}.turn_window == 0u);
  }
  if (!gpu) { std::printf("wfair scheduler: configure ok\n"); return 0; }

  std::vector<Endpoint> eps((size_t)P);
  std::vector<eppk_pod_row> rows((size_t)P);
  std::memset(rows.data(), 0, rows.size() * sizeof(eppk_pod_row));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < P; ++i) {
    eps[(size_t)i].address = "10.5.0." + std::to_string(i);
    eps[(size_t)i].port = "8000";
    rows[(size_t)i].queue = (uint32_t)(rnd() % 12);
    rows[(size_t)i].kv_util = (double)(rnd() % 1025) / 1024.0;
    rows[(size_t)i].max_lora = 4;
  }
  GpuPickerOptions go; go.max_pods = opt.max_pods; go.max_blocks = opt.max_blocks; go.max_batch = opt.max_batch;
  SchedulerProfile dp; dp.scorers = specs[0].scorers;
  eppk_cfg dcfg = MakeCfg(dp, go, opt.index_slots, 0);
  eppk_ctx* direct = nullptr;
  CHECK(eppk_create(&dcfg, &direct) == EPPK_OK);
  CHECK(eppk_snapshot_publish(direct, rows.data(), (uint32_t)P, 1) == EPPK_OK);
  const std::string model = "base";
  const int N = 100;                                                               // (one group: below max_batch; two chunks of 64 rows)
  std::vector<Request> reqs((size_t)N);
  for (int i = 0; i < N; ++i) {
    reqs[(size_t)i].request_id = "req-" + std::to_string(i);
    reqs[(size_t)i].target_model = model;
    reqs[(size_t)i].prompt = std::string((size_t)(i % 2 ? 40 : 300), (char)('a' + i % 7)) + std::to_string(i);
    reqs[(size_t)i].band = (uint8_t)(i % 10 == 9 ? 0 : 1);
    reqs[(size_t)i].flow = (uint16_t)(i % 3);
  }
  std::vector<uint8_t> rb, band((size_t)N);
  std::vector<uint16_t> flow((size_t)N);
  MakeRows(reqs, model, B, &rb);
  for (int i = 0; i < N; ++i) { band[(size_t)i] = reqs[(size_t)i].band; flow[(size_t)i] = reqs[(size_t)i].flow; }
  eppk_band_table table;
  std::memset(&table, 0, sizeof table);
  table.n_bands = 2;
  table.reserve[1] = 2;
  std::vector<int32_t> wp((size_t)N), fp((size_t)N);
  std::vector<double> ws((size_t)N), fs((size_t)N);
  std::vector<SchedulingResult> res;
  std::vector<Status> st;
  int differ = 0, shed = 0;
  {                                                                                // weights, no carry
    Scheduler sched;
    CHECK(sched.Configure(specs, &handler, opt).ok() && sched.PublishSnapshot(eps, rows, {}, 1).ok());
    CHECK(sched.Turns("decode").empty());
    CHECK(sched.ScheduleBatch(reqs, 0, &res, &st).ok() && res.size() == (size_t)N);
    CHECK(eppk_pick_wfair(direct, rb.data(), (uint32_t)N, nullptr, specs[0].k, flow.data(), kFlows, weights.data(), nullptr, nullptr, band.data(), &table, nullptr,
                          specs[0].cap_all, nullptr, wp.data(), ws.data(), nullptr) == EPPK_OK);
    CHECK(eppk_pick_fair(direct, rb.data(), (uint32_t)N, nullptr, specs[0].k, flow.data(), kFlows, nullptr, band.data(), &table, nullptr, specs[0].cap_all, nullptr,
                         fp.data(), fs.data(), nullptr) == EPPK_OK);
    CHECK(SamePicks(res, st, wp, eps));
    int placed[3] = {0, 0, 0};
    for (int i = 0; i < N; ++i) {
      differ += wp[(size_t)i] != fp[(size_t)i];
      shed += wp[(size_t)i] < 0;
      if (wp[(size_t)i] >= 0) ++placed[i % 3];
    }
    CHECK(shed > 0 && differ > 0);                                                 // the caps bind, and the weights decide
    CHECK(placed[0] > placed[1] && placed[0] > placed[2]);
  }
  {                                                                                // weights and carried turns
    std::vector<ProfileSpec> carry = specs;
    carry[0].turn_window = 4;
    Scheduler sched;
    CHECK(sched.Configure(carry, &handler, opt).ok() && sched.PublishSnapshot(eps, rows, {}, 1).ok());
    std::vector<uint32_t> turns(2u * kFlows, 0u);
    CHECK(sched.Turns("decode") == turns);
    std::vector<int32_t> first;
    for (int batch = 0; batch < 3; ++batch) {
      CHECK(sched.ScheduleBatch(reqs, 0, &res, &st).ok());
      CHECK(eppk_pick_wfair(direct, rb.data(), (uint32_t)N, nullptr, specs[0].k, flow.data(), kFlows, weights.data(), turns.data(), nullptr, band.data(), &table,
                            nullptr, specs[0].cap_all, nullptr, wp.data(), ws.data(), nullptr) == EPPK_OK);
      CHECK(eppk_fair_turns_rebase(turns.data(), weights.data(), 2, kFlows, 4) == EPPK_OK);
      CHECK(SamePicks(res, st, wp, eps));
      CHECK(sched.Turns("decode") == turns);
      if (batch == 0) first = wp;
    }
    int moved = 0;
    for (int i = 0; i < N; ++i) moved += first[(size_t)i] != wp[(size_t)i];
    CHECK(moved > 0);                                                              // the turns of earlier batches decide who is placed now
  }
  eppk_destroy(direct);
  std::printf("wfair scheduler: ok: %d requests; %d shed; %d picks differ from equal weights\n", N, shed, differ);
  return 0;
}
