// Test of the C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with a PickerKind::Bounded profile that has n_flows (SEMANTICS.md §3g).
// Without an argument (no device needed): Configure refuses n_flows on any other picker kind and more than EPPK_MAX_FLOWS, by profile
// name.  With `gpu`: a costed `decode` profile with two bands and nine flows, whose results must equal direct eppk_pick_fair calls on the
// same rows (a context of its own with the same chain, snapshot and index), pick for pick, and differ from eppk_pick_costed (the flows
// decide); n_flows without `costed` and without `bands` is eppk_pick_fair with a null cost and one band; a request whose flow is
// >= n_flows gets an Internal status of its own and the batch goes on without it.
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

static void MakeRows(const std::vector<Request>& reqs, size_t lo, uint32_t m, const std::string& model, int B, std::vector<uint8_t>* rb) {
  const size_t stride = 8u + 8u * (size_t)B;
  rb->assign((size_t)m * stride, 0);
  for (uint32_t i = 0; i < m; ++i) {
    const Request& rq = reqs[lo + i];
    eppk_req_hdr hdr; hdr.adapter = -1;
    hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)rq.prompt.data(), rq.prompt.size(), 64,
                                              (uint64_t*)(rb->data() + (size_t)i * stride + 8), (uint32_t)B);
    std::memcpy(rb->data() + (size_t)i * stride, &hdr, 8);
  }
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  const int P = 12, B = 8;
  const uint32_t kFlows = 9;
  std::vector<ProfileSpec> specs(1);
  specs[0].name = "decode";
  specs[0].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_KV, 5}};
  specs[0].picker = PickerKind::Bounded;
  specs[0].k = 3;
  specs[0].cap_all = 20;                                                           // cost units
  specs[0].costed = true;
  specs[0].n_flows = kFlows;
  specs[0].bands = {{EPPK_BOUNDED_SHED, 0}, {EPPK_BOUNDED_SHED, 6}};
  OneProfile handler;
  Scheduler::Options opt;
  opt.max_pods = 64; opt.max_blocks = B; opt.max_batch = 128;                      // (smaller than the batch: the groups are chunked)
  opt.index_slots = 1024;
  {                                                                                // refused before any context is created
    std::vector<ProfileSpec> bad = specs;
    bad[0].bands.clear();
    bad[0].costed = false;
    for (PickerKind kind : {PickerKind::BestScore, PickerKind::RandomTopK, PickerKind::WeightedRandom}) {
      bad[0].picker = kind;
      Scheduler refused;
      const Status rs = refused.Configure(bad, &handler, opt);
      CHECK(!rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find("n_flows") != std::string::npos);
    }
    bad[0].picker = PickerKind::Bounded;
    bad[0].n_flows = EPPK_MAX_FLOWS + 1u;
    Scheduler refused;
    const Status rs = refused.Configure(bad, &handler, opt);
    CHECK(!rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find("flows") != std::string::npos);
    Request rq;
    CHECK(rq.flow == 0u && ProfileSpec{}.n_flows == 0u);
  }
  if (!gpu) { std::printf("fair scheduler: configure ok\n"); return 0; }

  std::vector<Endpoint> eps((size_t)P);
  std::vector<eppk_pod_row> rows((size_t)P);
  std::memset(rows.data(), 0, rows.size() * sizeof(eppk_pod_row));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < P; ++i) {
    eps[(size_t)i].address = "10.4.0." + std::to_string(i);
    eps[(size_t)i].port = "8000";
    rows[(size_t)i].queue = (uint32_t)(rnd() % 12);
    rows[(size_t)i].kv_util = (double)(rnd() % 1025) / 1024.0;
    rows[(size_t)i].max_lora = 4;
  }
  Scheduler sched;
  CHECK(sched.Configure(specs, &handler, opt).ok());
  CHECK(sched.PublishSnapshot(eps, rows, {}, 1).ok());
  GpuPickerOptions go; go.max_pods = opt.max_pods; go.max_blocks = opt.max_blocks; go.max_batch = opt.max_batch;
  SchedulerProfile dp; dp.scorers = specs[0].scorers;
  eppk_cfg dcfg = MakeCfg(dp, go, opt.index_slots, 0);
  eppk_ctx* direct = nullptr;
  CHECK(eppk_create(&dcfg, &direct) == EPPK_OK);
  CHECK(eppk_snapshot_publish(direct, rows.data(), (uint32_t)P, 1) == EPPK_OK);
  uint32_t geo[2] = {0, 0};                                                        // the driver sets EPPK_BOUND_CHUNK=64: a full group of 128
  CHECK(eppk_bounded_geometry(direct, geo) == EPPK_OK && geo[0] < opt.max_batch);  // requests is two chunks, the last group less than one
  const std::string model = "base";
  const int N = 150;
  std::vector<Request> reqs((size_t)N);
  for (int i = 0; i < N; ++i) {
    reqs[(size_t)i].request_id = "req-" + std::to_string(i);
    reqs[(size_t)i].target_model = model;
    reqs[(size_t)i].prompt = std::string((size_t)(i % 2 ? 40 : 300), (char)('a' + i % 7)) + std::to_string(i);
    reqs[(size_t)i].band = (uint8_t)(i % 10 == 9 ? 0 : 1);
    reqs[(size_t)i].cost = 1u + (uint32_t)(i % 5);
    reqs[(size_t)i].flow = (uint16_t)(i < 90 ? 0 : 1 + i % 8);                     // one tenant in front of everybody else
  }
  std::vector<SchedulingResult> res;
  std::vector<Status> st;
  CHECK(sched.ScheduleBatch(reqs, 0, &res, &st).ok());
  CHECK(res.size() == (size_t)N);

  eppk_band_table table;
  std::memset(&table, 0, sizeof table);
  table.n_bands = 2;
  table.reserve[1] = 6;
  int shed = 0, differ = 0;
  for (size_t lo = 0; lo < (size_t)N; lo += opt.max_batch) {
    const uint32_t m = (uint32_t)std::min<size_t>(opt.max_batch, (size_t)N - lo);
    std::vector<uint8_t> rb, band(m), rank(m);
    std::vector<uint32_t> cost(m);
    std::vector<uint16_t> flow(m);
    MakeRows(reqs, lo, m, model, B, &rb);
    for (uint32_t i = 0; i < m; ++i) { band[i] = reqs[lo + i].band; cost[i] = reqs[lo + i].cost; flow[i] = reqs[lo + i].flow; }
    std::vector<int32_t> op(m), cp(m);
    std::vector<double> os(m), cs(m);
    CHECK(eppk_pick_fair(direct, rb.data(), m, nullptr, specs[0].k, flow.data(), kFlows, cost.data(), band.data(), &table, nullptr, specs[0].cap_all, nullptr,
                         op.data(), os.data(), rank.data()) == EPPK_OK);
    CHECK(eppk_pick_costed(direct, rb.data(), m, nullptr, specs[0].k, cost.data(), band.data(), &table, nullptr, specs[0].cap_all, nullptr, cp.data(), cs.data(),
                           nullptr) == EPPK_OK);
    std::vector<uint32_t> taken((size_t)P, 0);
    for (uint32_t i = 0; i < m; ++i) {
      const SchedulingResult& sr = res[lo + i];
      auto it = sr.profile_results.find("decode");
      CHECK(it != sr.profile_results.end());
      CHECK((op[i] >= 0) == (rank[i] < specs[0].k));
      if (cp[i] != op[i]) ++differ;
      if (op[i] < 0) {                                                   // shed: no endpoint, Unavailable
        CHECK(it->second.empty() && st[lo + i].code == Code::Unavailable);
        ++shed;
        continue;
      }
      CHECK(it->second.size() == 1 && it->second[0]->address == eps[(size_t)op[i]].address && st[lo + i].ok());
      taken[(size_t)op[i]] += cost[i];
      CHECK(taken[(size_t)op[i]] <= specs[0].cap_all - (band[i] ? 6u : 0u));
    }
  }
  CHECK(shed > 0 && differ > 0);                                                   // the caps bind, and the flows decide

  std::vector<Request> few(reqs.begin(), reqs.begin() + 100);
  {                                                                                // no bands, no costs: one band with bounded_policy, count units
    std::vector<ProfileSpec> plain = specs;
    plain[0].bands.clear();
    plain[0].costed = false;
    plain[0].cap_all = 5;
    plain[0].bounded_policy = EPPK_BOUNDED_SHED;
    Scheduler s2;
    CHECK(s2.Configure(plain, &handler, opt).ok() && s2.PublishSnapshot(eps, rows, {}, 1).ok());
    std::vector<SchedulingResult> r2;
    std::vector<Status> st2;
    CHECK(s2.ScheduleBatch(few, 0, &r2, &st2).ok());
    std::vector<uint8_t> rb;
    std::vector<uint16_t> flow(few.size());
    MakeRows(few, 0, (uint32_t)few.size(), model, B, &rb);
    for (size_t i = 0; i < few.size(); ++i) flow[i] = few[i].flow;
    eppk_band_table one;
    std::memset(&one, 0, sizeof one);
    one.n_bands = 1; one.policy[0] = EPPK_BOUNDED_SHED;
    std::vector<int32_t> pp(few.size());
    std::vector<double> ps(few.size());
    CHECK(eppk_pick_fair(direct, rb.data(), (uint32_t)few.size(), nullptr, 3, flow.data(), kFlows, nullptr, nullptr, &one, nullptr, 5, nullptr, pp.data(),
                         ps.data(), nullptr) == EPPK_OK);
    int placed_late = 0;
    for (size_t i = 0; i < few.size(); ++i) {
      const auto& v = r2[i].profile_results.at("decode");
      CHECK(pp[i] < 0 ? (v.empty() && st2[i].code == Code::Unavailable) : (v.size() == 1 && v[0]->address == eps[(size_t)pp[i]].address && st2[i].ok()));
      placed_late += i >= 90 && pp[i] >= 0;
    }
    CHECK(placed_late == 10);                                                      // at least 15 slots in reach of everybody: the ten requests behind the tenant are in the first 12 places
  }
  {                                                                                // a flow out of range: that request's own Internal status
    std::vector<Request> bad = few;
    bad[4].flow = (uint16_t)kFlows;
    bad[50].flow = 0xFFFF;
    std::vector<Request> rest;
    for (size_t i = 0; i < bad.size(); ++i) if (i != 4 && i != 50) rest.push_back(bad[i]);
    std::vector<SchedulingResult> r3;
    std::vector<Status> st3;
    CHECK(sched.ScheduleBatch(bad, 0, &r3, &st3).ok());
    CHECK(st3[4].code == Code::Internal && st3[4].message.find("flow 9") != std::string::npos && r3[4].profile_results.at("decode").empty());
    CHECK(st3[50].code == Code::Internal && st3[50].message.find("decode") != std::string::npos && r3[50].profile_results.at("decode").empty());
    std::vector<uint8_t> rb, band(rest.size());
    std::vector<uint32_t> cost(rest.size());
    std::vector<uint16_t> flow(rest.size());
    MakeRows(rest, 0, (uint32_t)rest.size(), model, B, &rb);
    for (size_t i = 0; i < rest.size(); ++i) { band[i] = rest[i].band; cost[i] = rest[i].cost; flow[i] = rest[i].flow; }
    std::vector<int32_t> pp(rest.size());
    std::vector<double> ps(rest.size());
    CHECK(eppk_pick_fair(direct, rb.data(), (uint32_t)rest.size(), nullptr, 3, flow.data(), kFlows, cost.data(), band.data(), &table, nullptr, specs[0].cap_all,
                         nullptr, pp.data(), ps.data(), nullptr) == EPPK_OK);
    for (size_t i = 0, q = 0; i < bad.size(); ++i) {
      if (i == 4 || i == 50) continue;
      const auto& v = r3[i].profile_results.at("decode");
      CHECK(pp[q] < 0 ? (v.empty() && st3[i].code == Code::Unavailable) : (v.size() == 1 && v[0]->address == eps[(size_t)pp[q]].address && st3[i].ok()));
      ++q;
    }
  }
  eppk_destroy(direct);
  std::printf("fair scheduler: ok: %d requests; %d shed; %d picks differ from batch order\n", N, shed, differ);
  return 0;
}
