// Test of the C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with priority bands on a PickerKind::Bounded profile (SEMANTICS.md
// §3e).  Without an argument (no device needed): Configure refuses more than 8 bands and decreasing reserves, by profile name.  With
// `gpu`: a `decode` profile with three bands behind a metric predicate, whose results must equal direct eppk_filter_masks +
// eppk_pick_banded calls on the same rows (a context of its own with the same chain, snapshot, index and program), pick for pick; a
// request the picker sheds ends as Unavailable; the critical band is shed last; an empty `bands` takes eppk_pick_bounded as before; a
// request whose band the table does not have fails the batch.
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

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  const int P = 40, B = 8;
  std::vector<ProfileSpec> specs(1);
  specs[0].name = "decode";
  specs[0].scorers = {{EPPK_SCORER_PREFIX, 3}, {EPPK_SCORER_KV, 5}};
  specs[0].picker = PickerKind::Bounded;
  specs[0].k = 3;
  specs[0].cap_all = 2;
  specs[0].bands = {{EPPK_BOUNDED_SHED, 0}, {EPPK_BOUNDED_SHED, 0}, {EPPK_BOUNDED_SHED, 1}};   // critical, standard, sheddable (one slot held back)
  eppk_predicate pred;
  std::memset(&pred, 0, sizeof pred);
  pred.kind = EPPK_PRED_QUEUE_LE; pred.on_empty = EPPK_ON_EMPTY_REQUIRE; pred.u = 9;
  specs[0].predicates = {pred};
  OneProfile handler;
  Scheduler::Options opt;
  opt.max_pods = 64; opt.max_blocks = B; opt.max_batch = 128;                      // (smaller than the batch: the groups are chunked)
  opt.index_slots = 1024;
  {                                                                                // refused before any context is created
    std::vector<ProfileSpec> bad = specs;
    bad[0].bands.assign(9, eppk_band{});
    Scheduler refused;
    Status rs = refused.Configure(bad, &handler, opt);
    CHECK(!rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find("8 bands") != std::string::npos);
    bad[0].bands = {{EPPK_BOUNDED_SHED, 2}, {EPPK_BOUNDED_SPILL, 1}};
    rs = refused.Configure(bad, &handler, opt);
    CHECK(!rs.ok() && rs.message.find("decode") != std::string::npos && rs.message.find("reserve of band 1") != std::string::npos);
  }
  if (!gpu) { std::printf("banded scheduler: configure ok\n"); return 0; }

  std::vector<Endpoint> eps((size_t)P);
  std::vector<eppk_pod_row> rows((size_t)P);
  std::memset(rows.data(), 0, rows.size() * sizeof(eppk_pod_row));
  uint64_t x = 0x2545F4914F6CDD1Dull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int i = 0; i < P; ++i) {
    eps[(size_t)i].address = "10.3.0." + std::to_string(i);
    eps[(size_t)i].port = "8000";
    rows[(size_t)i].queue = (uint32_t)(rnd() % 12);
    rows[(size_t)i].kv_util = (double)(rnd() % 1025) / 1024.0;
    rows[(size_t)i].max_lora = 4;
  }
  Scheduler sched;
  CHECK(sched.Configure(specs, &handler, opt).ok());
  CHECK(sched.PublishSnapshot(eps, rows, {}, 1).ok());
  // the profile again, as a context of its own: the direct calls the scheduler's results must equal
  GpuPickerOptions go; go.max_pods = opt.max_pods; go.max_blocks = opt.max_blocks; go.max_batch = opt.max_batch;
  SchedulerProfile dp; dp.scorers = specs[0].scorers;
  eppk_cfg dcfg = MakeCfg(dp, go, opt.index_slots, 0);
  eppk_ctx* direct = nullptr;
  CHECK(eppk_create(&dcfg, &direct) == EPPK_OK);
  CHECK(eppk_snapshot_publish(direct, rows.data(), (uint32_t)P, 1) == EPPK_OK);
  eppk_filter_program prog;
  std::memset(&prog, 0, sizeof prog);
  prog.n_stages = 1; prog.stage[0] = pred;
  CHECK(eppk_set_filters(direct, &prog, 1) == EPPK_OK);
  uint32_t geo[2] = {0, 0};                                                        // the driver sets EPPK_BOUND_CHUNK=64: a full group of 128
  CHECK(eppk_bounded_geometry(direct, geo) == EPPK_OK && geo[1] < opt.max_batch);  // requests takes the band order and the launches per band
  const std::string model = "base";
  std::vector<std::string> sys;
  for (int g = 0; g < 5; ++g) sys.push_back(std::string(256, (char)('A' + g)));
  for (int g = 0; g < 5; ++g) {
    uint64_t h[8];
    const int n = eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)sys[(size_t)g].data(), sys[(size_t)g].size(), 64, h, 8);
    CHECK(n == 4);
    for (int pod : {g * 6, g * 6 + 1, g * 6 + 2})
      for (int i = 0; i < n; ++i) {
        const uint32_t pp = (uint32_t)pod;
        CHECK(sched.IndexInsert("decode", &h[i], &pp, 1).ok());
        CHECK(eppk_index_insert(direct, &h[i], &pp, 1) == EPPK_OK);
      }
  }
  const int N = 150;
  std::vector<Request> reqs((size_t)N);
  for (int i = 0; i < N; ++i) {
    reqs[(size_t)i].request_id = "req-" + std::to_string(i);
    reqs[(size_t)i].target_model = model;
    reqs[(size_t)i].prompt = sys[(size_t)(i % 5)] + std::string((size_t)(i % 2 ? 40 : 300), (char)('a' + i % 7)) + std::to_string(i);
    reqs[(size_t)i].band = (uint8_t)(i % 10 == 9 ? 0 : i % 10 < 6 ? 1 : 2);        // critical requests sit at the END of every ten
  }
  std::vector<SchedulingResult> res;
  std::vector<Status> st;
  CHECK(sched.ScheduleBatch(reqs, 0, &res, &st).ok());
  CHECK(res.size() == (size_t)N);

  const size_t stride = 8u + 8u * (size_t)B;
  eppk_band_table table;
  std::memset(&table, 0, sizeof table);
  table.n_bands = 3;
  table.reserve[2] = 1;
  int shed[3] = {0, 0, 0}, total[3] = {0, 0, 0}, plain_shed0 = 0, differ = 0;
  for (size_t lo = 0; lo < (size_t)N; lo += opt.max_batch) {
    const uint32_t m = (uint32_t)std::min<size_t>(opt.max_batch, (size_t)N - lo);
    std::vector<uint8_t> rb((size_t)m * stride, 0), band(m), rank(m);
    for (uint32_t i = 0; i < m; ++i) {
      const Request& rq = reqs[lo + i];
      eppk_req_hdr hdr; hdr.adapter = -1;
      hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)rq.prompt.data(), rq.prompt.size(), 64,
                                                (uint64_t*)(rb.data() + (size_t)i * stride + 8), B);
      std::memcpy(rb.data() + (size_t)i * stride, &hdr, 8);
      band[i] = rq.band;
    }
    std::vector<int32_t> op(m), pp(m);
    std::vector<double> os(m), ps(m);
    std::vector<uint64_t> fmask((size_t)m * ((P + 63) / 64));
    CHECK(eppk_filter_masks(direct, rb.data(), m, nullptr, nullptr, fmask.data(), nullptr) == EPPK_OK);
    CHECK(eppk_pick_banded(direct, rb.data(), m, fmask.data(), specs[0].k, band.data(), &table, nullptr, specs[0].cap_all, nullptr, op.data(), os.data(),
                           rank.data()) == EPPK_OK);
    CHECK(eppk_pick_bounded(direct, rb.data(), m, fmask.data(), specs[0].k, nullptr, specs[0].cap_all, EPPK_BOUNDED_SHED, nullptr, pp.data(), ps.data(),
                            nullptr) == EPPK_OK);
    std::vector<int> taken((size_t)P, 0);
    for (uint32_t i = 0; i < m; ++i) {
      const SchedulingResult& sr = res[lo + i];
      auto it = sr.profile_results.find("decode");
      CHECK(it != sr.profile_results.end());
      CHECK((op[i] >= 0) == (rank[i] < specs[0].k));
      ++total[band[i]];
      if (pp[i] < 0 && band[i] == 0) ++plain_shed0;
      if (pp[i] != op[i]) ++differ;
      if (op[i] < 0) {                                                   // shed: no endpoint, Unavailable
        CHECK(it->second.empty() && st[lo + i].code == Code::Unavailable);
        ++shed[band[i]];
        continue;
      }
      CHECK(it->second.size() == 1 && it->second[0]->address == eps[(size_t)op[i]].address && st[lo + i].ok());
      CHECK(++taken[(size_t)op[i]] <= (int)specs[0].cap_all && rows[(size_t)op[i]].queue <= 9);
    }
  }
  // the caps bind, the bands decide, and the critical band is shed last: batch order alone sheds more of it
  CHECK(shed[1] + shed[2] > 0 && differ > 0 && shed[0] < plain_shed0);
  CHECK(shed[0] * total[2] <= shed[2] * total[0]);

  {                                                                                // no bands: today's path, pick for pick
    std::vector<ProfileSpec> plain = specs;
    plain[0].bands.clear();
    Scheduler s2;
    CHECK(s2.Configure(plain, &handler, opt).ok() && s2.PublishSnapshot(eps, rows, {}, 1).ok());
    std::vector<Request> few(reqs.begin(), reqs.begin() + 100);
    std::vector<SchedulingResult> r2;
    std::vector<Status> st2;
    CHECK(s2.ScheduleBatch(few, 0, &r2, &st2).ok());
    std::vector<uint8_t> rb(few.size() * stride, 0);
    for (size_t i = 0; i < few.size(); ++i) {
      eppk_req_hdr hdr; hdr.adapter = -1;
      hdr.n_blocks = (uint32_t)eppk_hash_prompt((const uint8_t*)model.data(), model.size(), (const uint8_t*)few[i].prompt.data(), few[i].prompt.size(), 64,
                                                (uint64_t*)(rb.data() + i * stride + 8), B);
      std::memcpy(rb.data() + i * stride, &hdr, 8);
    }
    eppk_ctx* d2 = nullptr;
    CHECK(eppk_create(&dcfg, &d2) == EPPK_OK && eppk_snapshot_publish(d2, rows.data(), (uint32_t)P, 1) == EPPK_OK && eppk_set_filters(d2, &prog, 1) == EPPK_OK);
    std::vector<uint64_t> fmask(few.size() * ((P + 63) / 64));
    std::vector<int32_t> pp(few.size());
    std::vector<double> ps(few.size());
    CHECK(eppk_filter_masks(d2, rb.data(), (uint32_t)few.size(), nullptr, nullptr, fmask.data(), nullptr) == EPPK_OK);
    CHECK(eppk_pick_bounded(d2, rb.data(), (uint32_t)few.size(), fmask.data(), 3, nullptr, 2, EPPK_BOUNDED_SHED, nullptr, pp.data(), ps.data(), nullptr) == EPPK_OK);
    for (size_t i = 0; i < few.size(); ++i) {
      const auto& v = r2[i].profile_results.at("decode");
      CHECK(pp[i] < 0 ? v.empty() : (v.size() == 1 && v[0]->address == eps[(size_t)pp[i]].address));
    }
    eppk_destroy(d2);
  }
  {                                                                                // a band the table does not have fails the batch
    std::vector<Request> few(reqs.begin(), reqs.begin() + 10);
    few[4].band = 3;
    std::vector<SchedulingResult> r3;
    std::vector<Status> st3;
    const Status rs = sched.ScheduleBatch(few, 0, &r3, &st3);
    CHECK(!rs.ok() && rs.message.find("row 4") != std::string::npos && rs.message.find("band 3") != std::string::npos);
  }
  eppk_destroy(direct);
  std::printf("banded scheduler: ok: %d requests; shed per band %d/%d, %d/%d, %d/%d; batch order alone sheds %d of the critical band; %d picks differ\n", N,
              shed[0], total[0], shed[1], total[1], shed[2], total[2], plain_shed0, differ);
  return 0;
}
