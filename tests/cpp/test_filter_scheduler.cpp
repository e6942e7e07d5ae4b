// GPU test of the C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with metric predicates (SEMANTICS.md §2c; ProfileSpec::predicates):
// the two profiles of docs/proposals/0845-scheduler-architecture-proposal/examples/example.yaml, `decode` with best-score behind
// [KV_LE 0.5 REQUIRE, LORA_LOADED REQUIRE, QUEUE_WITHIN 3 PREFER] and `prefill` with PickerKind::WeightedRandom behind [KV_LE 0.75 REQUIRE].
// The cycle runs twice: the second time `prefill` samples with PickerKind::RandomTopK (k = 3) behind the same predicates.
// Each profile's results must equal DIRECT calls on a context of its own with the same chain, snapshot, index and programs --
// eppk_pick_filtered for decode, eppk_filter_masks + eppk_pick_weighted_random / eppk_pick_random_topk for prefill -- and a request the decode predicates shed
// (its adapter is loaded on no decode pod) must come back Unavailable.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gateway-api-inference-extension_amd/host/eppk_host.hpp"

using namespace eppk_host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static eppk_predicate pred(uint32_t kind, uint32_t on_empty, uint32_t u, double f) {
  eppk_predicate p;
  std::memset(&p, 0, sizeof p);
  p.kind = kind; p.on_empty = on_empty; p.u = u; p.f = f;
  return p;
}

static int run(PickerKind prefill_picker) {
  const int P = 120, B = 8;
  std::vector<Endpoint> eps((size_t)P);
  std::vector<eppk_pod_row> rows((size_t)P);
  std::memset(rows.data(), 0, rows.size() * sizeof(eppk_pod_row));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < P; ++i) {
    eps[(size_t)i].address = "10.3.0." + std::to_string(i);
    eps[(size_t)i].port = "8000";
    eps[(size_t)i].labels["role"] = (i % 3 == 0) ? "prefill" : "decode";
    rows[(size_t)i].queue = (uint32_t)(rnd() % 12);
    rows[(size_t)i].running = (uint32_t)(rnd() % 9);
    rows[(size_t)i].kv_util = (double)(rnd() % 1025) / 1024.0;
    rows[(size_t)i].max_lora = 4;
    if (i % 4 == 1) rows[(size_t)i].active[0] |= 1ull << 3;               // adapter 3 ("lora-a") runs on a quarter of the pods; adapter 5 nowhere
  }
  std::vector<ProfileSpec> specs(2);
  specs[0].name = "prefill";
  specs[0].filter = [](const Endpoint& e) { return e.labels.at("role") == "prefill"; };
  specs[0].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_QUEUE, 2}};
  specs[0].picker = prefill_picker;
  specs[0].k = 3;
  specs[0].predicates = {pred(EPPK_PRED_KV_LE, EPPK_ON_EMPTY_REQUIRE, 0, 0.75)};
  specs[1].name = "decode";
  specs[1].filter = [](const Endpoint& e) { return e.labels.at("role") == "decode"; };
  specs[1].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_KV, 5}};
  specs[1].picker = PickerKind::BestScore;
  specs[1].predicates = {pred(EPPK_PRED_KV_LE, EPPK_ON_EMPTY_REQUIRE, 0, 0.5), pred(EPPK_PRED_LORA_LOADED, EPPK_ON_EMPTY_REQUIRE, 0, 0.0),
                         pred(EPPK_PRED_QUEUE_WITHIN, EPPK_ON_EMPTY_PREFER, 3, 0.0)};
  DisaggTokenLengthHandler handler("prefill", "decode", 400);
  Scheduler sched;
  Scheduler::Options opt;
  opt.max_pods = 128; opt.max_blocks = B; opt.max_batch = 64;                      // (smaller than the batch: the groups are chunked)
  opt.index_slots = 1024;
  CHECK(sched.Configure(specs, &handler, opt).ok());
  const std::unordered_map<std::string, int32_t> adapters = {{"lora-a", 3}, {"lora-x", 5}};
  CHECK(sched.PublishSnapshot(eps, rows, adapters, 1).ok());

  // a program of five stages is refused at Configure, with the profile named
  {
    std::vector<ProfileSpec> bad = specs;
    bad[1].predicates.assign(5, pred(EPPK_PRED_QUEUE_LE, EPPK_ON_EMPTY_PREFER, 1, 0.0));
    Scheduler s2;
    const Status st2 = s2.Configure(bad, &handler, opt);
    CHECK(!st2.ok() && st2.message.find("decode") != std::string::npos);
  }

  // each profile again, as a context of its own: the direct calls the scheduler's results must equal
  GpuPickerOptions go; go.max_pods = opt.max_pods; go.max_blocks = opt.max_blocks; go.max_batch = opt.max_batch;
  eppk_ctx* direct[2] = {nullptr, nullptr};
  for (int pi = 0; pi < 2; ++pi) {
    SchedulerProfile dp; dp.scorers = specs[(size_t)pi].scorers;
    eppk_cfg dcfg = MakeCfg(dp, go, opt.index_slots, 0);
    CHECK(eppk_create(&dcfg, &direct[pi]) == EPPK_OK);
    std::vector<eppk_pod_row> prow = rows;
    for (int i = 0; i < P; ++i)
      if (!specs[(size_t)pi].filter(eps[(size_t)i])) prow[(size_t)i].flags |= EPPK_POD_INACTIVE;
    CHECK(eppk_snapshot_publish(direct[pi], prow.data(), (uint32_t)P, 1) == EPPK_OK);
    eppk_filter_program prog;
    std::memset(&prog, 0, sizeof prog);
    prog.n_stages = (uint32_t)specs[(size_t)pi].predicates.size();
    for (size_t s = 0; s < specs[(size_t)pi].predicates.size(); ++s) prog.stage[s] = specs[(size_t)pi].predicates[s];
    CHECK(eppk_set_filters(direct[pi], &prog, 1) == EPPK_OK);
  }
  std::vector<std::string> sys;
  for (int g = 0; g < 5; ++g) sys.push_back(std::string(256, (char)('A' + g)));
  const std::string models[3] = {"base", "lora-a", "lora-x"};
  for (int g = 0; g < 5; ++g)
    for (const std::string& model : models) {
      uint64_t h[8];
      const int n = eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)sys[(size_t)g].data(), sys[(size_t)g].size(), 64, h, 8);
      CHECK(n == 4);
      for (int pod : {g * 6, g * 6 + 1, g * 6 + 2, g * 6 + 3, 90 + g})
        for (int pi = 0; pi < 2; ++pi)
          for (int i = 0; i < n; ++i) {
            const uint32_t pp = (uint32_t)pod;
            CHECK(sched.IndexInsert(specs[(size_t)pi].name, &h[i], &pp, 1).ok());
            CHECK(eppk_index_insert(direct[pi], &h[i], &pp, 1) == EPPK_OK);
          }
    }

  const int N = 150;
  std::vector<Request> reqs((size_t)N);
  for (int i = 0; i < N; ++i) {
    reqs[(size_t)i].request_id = "req-" + std::to_string(i);
    reqs[(size_t)i].target_model = models[i % 7 == 3 ? 2 : (i % 3 == 1 ? 1 : 0)];    // every seventh request asks for the adapter nobody holds
    reqs[(size_t)i].prompt = sys[(size_t)(i % 5)] + std::string((size_t)(i % 2 ? 40 : 300), (char)('a' + i % 7)) + std::to_string(i);   // short / long
  }
  const uint64_t seed = 20261018ull;
  std::vector<SchedulingResult> res;
  std::vector<Status> st;
  CHECK(sched.ScheduleBatch(reqs, seed, &res, &st).ok());
  CHECK(res.size() == (size_t)N);

  const size_t stride = 8u + 8u * (size_t)B;
  int n_prefill = 0, n_shed = 0, n_narrowed = 0;
  for (int pi = 0; pi < 2; ++pi) {
    std::vector<int> group;
    for (int i = 0; i < N; ++i)
      if (pi == 1 || reqs[(size_t)i].prompt.size() >= 400) group.push_back(i);
    if (pi == 0) n_prefill = (int)group.size();
    for (size_t lo = 0; lo < group.size(); lo += opt.max_batch) {
      const uint32_t m = (uint32_t)std::min<size_t>(opt.max_batch, group.size() - lo);
      std::vector<uint8_t> rb((size_t)m * stride, 0);
      for (uint32_t i = 0; i < m; ++i) {
        const Request& rq = reqs[(size_t)group[lo + i]];
        eppk_req_hdr hdr;
        auto it = adapters.find(rq.target_model);
        hdr.adapter = it == adapters.end() ? EPPK_ADAPTER_BASE : it->second;
        hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)rq.target_model.data(), rq.target_model.size(), (const uint8_t*)rq.prompt.data(),
                                                  rq.prompt.size(), 64, (uint64_t*)(rb.data() + (size_t)i * stride + 8), B);
        std::memcpy(rb.data() + (size_t)i * stride, &hdr, 8);
      }
      std::vector<int32_t> op(m);
      std::vector<double> os(m);
      std::vector<uint8_t> verdict(m, 0xEE);
      const size_t J = ((size_t)P + 63u) / 64u;
      std::vector<uint64_t> fm((size_t)m * J);
      if (pi == 1) {
        CHECK(eppk_pick_filtered(direct[pi], rb.data(), m, nullptr, nullptr, 1, op.data(), os.data(), verdict.data()) == EPPK_OK);
        CHECK(eppk_filter_masks(direct[pi], rb.data(), m, nullptr, nullptr, fm.data(), nullptr) == EPPK_OK);
      } else {
        CHECK(eppk_filter_masks(direct[pi], rb.data(), m, nullptr, nullptr, fm.data(), verdict.data()) == EPPK_OK);
        if (prefill_picker == PickerKind::WeightedRandom)
          CHECK(eppk_pick_weighted_random(direct[pi], rb.data(), m, fm.data(), 1, seed + lo, op.data(), os.data()) == EPPK_OK);
        else
          CHECK(eppk_pick_random_topk(direct[pi], rb.data(), m, fm.data(), 3, seed + lo, op.data(), os.data()) == EPPK_OK);
      }
      for (uint32_t i = 0; i < m; ++i) {
        const int r = group[lo + i];
        const SchedulingResult& sr = res[(size_t)r];
        auto it = sr.profile_results.find(specs[(size_t)pi].name);
        CHECK(it != sr.profile_results.end());
        if (op[i] < 0) {
          CHECK(it->second.empty());
          CHECK((verdict[i] & EPPK_VERDICT_SHED) != 0);
          if (pi == 1) { CHECK(st[(size_t)r].code == Code::Unavailable); CHECK(reqs[(size_t)r].target_model == "lora-x"); ++n_shed; }
          continue;
        }
        CHECK(it->second.size() == 1 && it->second[0] != nullptr);
        CHECK(it->second[0]->address == eps[(size_t)op[i]].address);
        CHECK(specs[(size_t)pi].filter(*it->second[0]));
        CHECK((fm[(size_t)i * J + (size_t)op[i] / 64u] >> ((size_t)op[i] % 64u)) & 1ull);          // the pick passed the predicates ...
        CHECK(rows[(size_t)op[i]].kv_util <= (pi == 1 ? 0.5 : 0.75));                                // ... which is what they say
        if (pi == 1) {
          CHECK(st[(size_t)r].ok());
          if (reqs[(size_t)r].target_model == "lora-a") { CHECK(rows[(size_t)op[i]].active[0] & (1ull << 3)); ++n_narrowed; }
        }
      }
    }
  }
  for (int i = 0; i < N; ++i) {
    CHECK(res[(size_t)i].primary_profile_name == "decode");
    CHECK((reqs[(size_t)i].target_model == "lora-x") == (st[(size_t)i].code == Code::Unavailable));
  }
  CHECK(n_prefill > 0 && n_prefill < N && n_shed > 10 && n_narrowed > 20);
  eppk_destroy(direct[0]); eppk_destroy(direct[1]);
  std::printf("%s prefill: %d requests, %d through prefill + decode, %d shed by the decode predicates (Unavailable), %d held to the pods "
              "that run their adapter; both profiles equal direct calls\n", prefill_picker == PickerKind::WeightedRandom ? "weighted-random" : "random-top-3",
              N, n_prefill, n_shed, n_narrowed);
  return 0;
}

int main() {
  if (run(PickerKind::WeightedRandom) != 0) return 1;
  if (run(PickerKind::RandomTopK) != 0) return 1;
  std::printf("filter scheduler ok\n");
  return 0;
}
