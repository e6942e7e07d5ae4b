// GPU test of the C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with the picker "best-score under per-pod caps" (SEMANTICS.md
// §3d): the two profiles of docs/proposals/0845-scheduler-architecture-proposal/examples/example.yaml, `prefill` with best-score (against
// the ORACLE, oracle/oracle.h) and `decode` with PickerKind::Bounded behind a metric predicate, whose results must equal direct
// eppk_filter_masks + eppk_pick_bounded calls on the same rows (a context of its own with the same chain, snapshot, index and program),
// pick for pick; a request the picker sheds for overflow ends as Unavailable.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gateway-api-inference-extension_amd/host/eppk_host.hpp"
#include "../../oracle/oracle.h"

using namespace eppk_host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main() {
  const int P = 120, B = 8;
  std::vector<Endpoint> eps((size_t)P);
  std::vector<eppk_pod_row> rows((size_t)P);
  std::memset(rows.data(), 0, rows.size() * sizeof(eppk_pod_row));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < P; ++i) {
    eps[(size_t)i].address = "10.2.0." + std::to_string(i);
    eps[(size_t)i].port = "8000";
    eps[(size_t)i].labels["role"] = (i % 3 == 0) ? "prefill" : "decode";          // is-prefill / is-decode filters
    eps[(size_t)i].labels["accelerator"] = (i % 5 == 0) ? "none" : "mi355x";     // has-required-accelerator
    rows[(size_t)i].queue = (uint32_t)(rnd() % 12);
    rows[(size_t)i].kv_util = (double)(rnd() % 1025) / 1024.0;
    rows[(size_t)i].max_lora = 4;
  }
  std::vector<ProfileSpec> specs(2);
  specs[0].name = "prefill";
  specs[0].filter = [](const Endpoint& e) { return e.labels.at("role") == "prefill" && e.labels.at("accelerator") == "mi355x"; };
  specs[0].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_QUEUE, 2}};           // (queue depth stands in for the example's latency-scorer)
  specs[0].picker = PickerKind::BestScore;
  specs[1].name = "decode";
  specs[1].filter = [](const Endpoint& e) { return e.labels.at("role") == "decode"; };
  specs[1].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_KV, 5}};              // example.yaml:21-23
  specs[1].picker = PickerKind::Bounded;
  specs[1].k = 3;
  specs[1].cap_all = 2;                                                            // per endpoint and batch handed to the library
  specs[1].bounded_policy = EPPK_BOUNDED_SHED;
  eppk_predicate pred;
  std::memset(&pred, 0, sizeof pred);
  pred.kind = EPPK_PRED_QUEUE_LE; pred.on_empty = EPPK_ON_EMPTY_REQUIRE; pred.u = 9;
  specs[1].predicates = {pred};
  DisaggTokenLengthHandler handler("prefill", "decode", 400);
  Scheduler sched;
  Scheduler::Options opt;
  opt.max_pods = 128; opt.max_blocks = B; opt.max_batch = 128;                     // (smaller than the batch: the groups are chunked)
  opt.index_slots = 1024;
  {                                                                                // a bounded profile without a cap is refused, by name
    std::vector<ProfileSpec> uncapped = specs;
    uncapped[1].cap_all = 0;
    Scheduler refused;
    const Status rs = refused.Configure(uncapped, &handler, opt);
    CHECK(!rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find("cap_all") != std::string::npos);
  }
  CHECK(sched.Configure(specs, &handler, opt).ok());
  CHECK(sched.PublishSnapshot(eps, rows, {}, 1).ok());

  // five system prompts, cached on a few pods of both roles
  std::vector<std::string> sys;
  for (int g = 0; g < 5; ++g) sys.push_back(std::string(256, (char)('A' + g)));
  orc_index* oix[2] = {orc_index_new(), orc_index_new()};
  // the decode profile again, as a context of its own: the direct calls the scheduler's decode results must equal
  GpuPickerOptions go; go.max_pods = opt.max_pods; go.max_blocks = opt.max_blocks; go.max_batch = opt.max_batch;
  SchedulerProfile dp; dp.scorers = specs[1].scorers;
  eppk_cfg dcfg = MakeCfg(dp, go, opt.index_slots, 0);
  eppk_ctx* direct = nullptr;
  CHECK(eppk_create(&dcfg, &direct) == EPPK_OK);
  std::vector<eppk_pod_row> prow[2] = {rows, rows};
  for (int pi = 0; pi < 2; ++pi)
    for (int i = 0; i < P; ++i)
      if (!specs[(size_t)pi].filter(eps[(size_t)i])) prow[pi][(size_t)i].flags |= EPPK_POD_INACTIVE;
  CHECK(eppk_snapshot_publish(direct, prow[1].data(), (uint32_t)P, 1) == EPPK_OK);
  eppk_filter_program prog;
  std::memset(&prog, 0, sizeof prog);
  prog.n_stages = 1; prog.stage[0] = pred;
  CHECK(eppk_set_filters(direct, &prog, 1) == EPPK_OK);
  uint32_t geo[2] = {0, 0};                                                        // the driver sets EPPK_BOUND_CHUNK=64: a full group of 128
  CHECK(eppk_bounded_geometry(direct, geo) == EPPK_OK && geo[1] < opt.max_batch);  // requests takes the launches-per-round form of the resolve
  const std::string model = "base";
  for (int g = 0; g < 5; ++g) {
    uint64_t h[8];
    const int n = eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)sys[(size_t)g].data(), sys[(size_t)g].size(), 64, h, 8);
    CHECK(n == 4);
    for (int pod : {g * 6, g * 6 + 1, g * 6 + 2, g * 6 + 3, 90 + g})
      for (int pi = 0; pi < 2; ++pi)
        for (int i = 0; i < n; ++i) {
          const uint32_t pp = (uint32_t)pod;
          CHECK(sched.IndexInsert(specs[(size_t)pi].name, &h[i], &pp, 1).ok());
          if (pi == 1) CHECK(eppk_index_insert(direct, &h[i], &pp, 1) == EPPK_OK);
          if (!(prow[pi][(size_t)pod].flags & EPPK_POD_INACTIVE)) orc_index_insert(oix[pi], h[i], pp);   // (a hole learns nothing: SEMANTICS.md 6b)
        }
  }

  const int N = 150;
  std::vector<Request> reqs((size_t)N);
  for (int i = 0; i < N; ++i) {
    reqs[(size_t)i].request_id = "req-" + std::to_string(i);
    reqs[(size_t)i].target_model = model;
    reqs[(size_t)i].prompt = sys[(size_t)(i % 5)] + std::string((size_t)(i % 2 ? 40 : 300), (char)('a' + i % 7)) + std::to_string(i);   // short / long
  }
  const uint64_t seed = 0;                                                        // (the bounded picker draws nothing)
  std::vector<SchedulingResult> res;
  std::vector<Status> st;
  CHECK(sched.ScheduleBatch(reqs, seed, &res, &st).ok());
  CHECK(res.size() == (size_t)N);

  // profile by profile, over the same groups in the same order and chunks: prefill against the oracle, decode against direct calls
  const size_t stride = 8u + 8u * (size_t)B;
  int n_prefill = 0, not_best = 0, shed = 0;
  for (int pi = 0; pi < 2; ++pi) {
    std::vector<int> group;
    for (int i = 0; i < N; ++i)
      if (pi == 1 || reqs[(size_t)i].prompt.size() >= 400) group.push_back(i);
    if (pi == 0) n_prefill = (int)group.size();
    eppk_weighted_scorer chain[2];
    for (int k = 0; k < 2; ++k) { chain[k].kind = (uint32_t)specs[(size_t)pi].scorers[(size_t)k].kind; chain[k].weight = specs[(size_t)pi].scorers[(size_t)k].weight; }
    for (size_t lo = 0; lo < group.size(); lo += opt.max_batch) {
      const uint32_t m = (uint32_t)std::min<size_t>(opt.max_batch, group.size() - lo);
      std::vector<uint8_t> rb((size_t)m * stride, 0);
      for (uint32_t i = 0; i < m; ++i) {
        const Request& rq = reqs[(size_t)group[lo + i]];
        eppk_req_hdr hdr; hdr.adapter = -1;
        hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)rq.prompt.data(), rq.prompt.size(), 64,
                                                  (uint64_t*)(rb.data() + (size_t)i * stride + 8), B);
        std::memcpy(rb.data() + (size_t)i * stride, &hdr, 8);
      }
      std::vector<int32_t> op(m), head(m);
      std::vector<double> os(m), hs(m);
      if (pi == 0) CHECK(orc_pick_batch(chain, 2, prow[pi].data(), P, oix[pi], rb.data(), B, m, nullptr, op.data(), os.data(), nullptr) == 0);
      else {
        std::vector<uint64_t> fmask((size_t)m * ((P + 63) / 64));
        std::vector<uint8_t> rank(m);
        CHECK(eppk_filter_masks(direct, rb.data(), m, nullptr, nullptr, fmask.data(), nullptr) == EPPK_OK);
        CHECK(eppk_pick_bounded(direct, rb.data(), m, fmask.data(), specs[1].k, nullptr, specs[1].cap_all, EPPK_BOUNDED_SHED, nullptr, op.data(), os.data(),
                                rank.data()) == EPPK_OK);
        CHECK(orc_pick_batch(chain, 2, prow[pi].data(), P, oix[pi], rb.data(), B, m, fmask.data(), head.data(), hs.data(), nullptr) == 0);
        std::vector<int> taken((size_t)P, 0);
        for (uint32_t i = 0; i < m; ++i) {
          CHECK((op[i] >= 0) == (rank[i] < specs[1].k));
          if (op[i] >= 0) CHECK(++taken[(size_t)op[i]] <= (int)specs[1].cap_all && rows[(size_t)op[i]].queue <= 9);
        }
      }
      for (uint32_t i = 0; i < m; ++i) {
        const SchedulingResult& sr = res[(size_t)group[lo + i]];
        auto it = sr.profile_results.find(specs[(size_t)pi].name);
        if (pi == 1 && op[i] < 0) {                                      // shed for overflow: no endpoint, Unavailable
          CHECK(it != sr.profile_results.end() && it->second.empty());
          CHECK(st[(size_t)group[lo + i]].code == Code::Unavailable);
          ++shed;
          continue;
        }
        CHECK(it != sr.profile_results.end() && it->second.size() == 1);
        CHECK(op[i] >= 0 && it->second[0] != nullptr);
        CHECK(it->second[0]->address == eps[(size_t)op[i]].address);
        CHECK(specs[(size_t)pi].filter(*it->second[0]));                 // the profile's filters hold
        if (pi == 1 && op[i] != head[i]) ++not_best;
      }
    }
  }
  for (int i = 0; i < N; ++i) {
    CHECK(res[(size_t)i].primary_profile_name == "decode");
    CHECK(st[(size_t)i].ok() == !res[(size_t)i].profile_results.at("decode").empty());
    CHECK(res[(size_t)i].profile_results.count("prefill") == (reqs[(size_t)i].prompt.size() >= 400 ? 1u : 0u));
  }
  CHECK(n_prefill > 0 && n_prefill < N && not_best > 0 && shed > 0 && shed < N);
  eppk_destroy(direct);
  orc_index_free(oix[0]); orc_index_free(oix[1]);
  std::printf("bounded scheduler ok: %d requests, %d through prefill + decode, %d bounded decode picks off the best-score pick, %d shed for "
              "overflow (Unavailable); decode equals direct eppk_pick_bounded calls\n", N, n_prefill, not_best, shed);
  return 0;
}
