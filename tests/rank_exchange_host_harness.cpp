// Host build of RankExchange (apex-solver_amd/csrc/rank_exchange.cpp over comm.cpp, both with APEX_COMM_HOST_ONLY: "device"
// buffers are host buffers, no HIP, no GPU) + two self-tests.  Built and driven by tests/test_rank_exchange_host.py under
// `pytest -m "not gpu"`: a RankExchange that is not active() touches nothing, and one ExchangeList issued between 2 and 3 real
// processes over the shared-memory transport gives the exact sums and the max.
#define APEX_COMM_HOST_ONLY 1
#include "../apex-solver_amd/csrc/comm.cpp"
#include "../apex-solver_amd/csrc/rank_exchange.cpp"

#include <stdio.h>

using apex::ExchangeItem;

// every call of a RankExchange, on buffers of a known pattern: all return kOk and leave the bytes as they were
static std::string idle_calls(apex::RankExchange& x) {
    if (x.active()) return "active()";
    double d[6], d0[6];
    int m[6], m0[6];
    for (int i = 0; i < 6; ++i) { d[i] = d0[i] = 1.5 + i; m[i] = m0[i] = 7 - i; }
    const int rc[] = {x.sum(d, 6, nullptr), x.max_int(m, 6, nullptr), x.reduce(d, 6, 0, nullptr), x.all_gather(d, d + 1, 8, nullptr),
                      x.broadcast(d, 6, 0, nullptr),
                      x.issue({{ExchangeItem::kSum, d, 6, -1}, {ExchangeItem::kSum, d, 3, 0}, {ExchangeItem::kSum, d, 0, -1}, {ExchangeItem::kMaxInt, m, 6, -1}}, nullptr)};
    for (size_t i = 0; i < sizeof rc / sizeof rc[0]; ++i) if (rc[i] != apex::kOk) return "call " + std::to_string(i) + " returned " + std::to_string(rc[i]);
    if (memcmp(d, d0, sizeof d) != 0 || memcmp(m, m0, sizeof m) != 0) return "a buffer was written";
    return "";
}

extern "C" int rank_exchange_idle_selftest(const char* name, char* msg, int msg_len) {
    auto fail = [&](const std::string& m) { snprintf(msg, (size_t)msg_len, "%s", m.c_str()); return 1; };
    std::string e;
    apex::RankExchange fresh;   // no communicator, world 1
    if (!(e = idle_calls(fresh)).empty()) return fail("fresh: " + e);
    apex::RankExchange shard;   // sharded, still no communicator
    if (shard.set_shard(1, 3) != apex::kOk || shard.rank() != 1 || shard.world() != 3 || shard.has_comm()) return fail("set_shard(1, 3)");
    if (!(e = idle_calls(shard)).empty()) return fail("sharded without a communicator: " + e);
    if (shard.set_shard(3, 3) != apex::kInvalidInput || shard.set_shard(-1, 2) != apex::kInvalidInput || shard.set_shard(0, 0) != apex::kInvalidInput)
        return fail("set_shard accepted a bad rank / world");
    if (shard.rank() != 1 || shard.world() != 3 || shard.error().empty()) return fail("a refused set_shard changed the shard or left no text");
    apex::RankExchange solo;    // a communicator of world 1
    std::string err;
    if (solo.set_shard(0, 1) != apex::kOk || solo.adopt(apex::make_shm_comm(1, 0, name, &err), err) != apex::kOk) return fail("world 1: " + solo.error());
    if (!solo.has_comm()) return fail("world 1: has_comm()");
    if (!(e = idle_calls(solo)).empty()) return fail("world 1 with a communicator: " + e);
    apex::RankExchange none;
    if (none.adopt(nullptr, "no transport") != apex::kDeviceError || none.error() != "no transport" || none.has_comm()) return fail("adopt(nullptr)");
    snprintf(msg, (size_t)msg_len, "idle ok");
    return 0;
}

// rank r of `world` contributes r + 1 in every slot of one list of four items
extern "C" int rank_exchange_list_selftest(int world, int rank, const char* name, char* msg, int msg_len) {
    auto fail = [&](const std::string& m) { snprintf(msg, (size_t)msg_len, "rank %d: %s", rank, m.c_str()); return 1; };
    apex::RankExchange x;
    std::string err;
    if (x.set_shard(rank, world) != apex::kOk) return fail("set_shard: " + x.error());
    if (x.adopt(apex::make_shm_comm(world, rank, name, &err), err) != apex::kOk) return fail("adopt: " + x.error());
    if (!x.active()) return fail("not active()");
    const double mine = (double)(rank + 1), total = 0.5 * world * (world + 1);
    double all[5], rooted[3];
    int mx[2] = {rank + 1, rank + 1};
    for (double& v : all) v = mine;
    for (double& v : rooted) v = mine;
    const int rc = x.issue({{ExchangeItem::kSum, all, 5, -1}, {ExchangeItem::kSum, rooted, 3, 1}, {ExchangeItem::kSum, nullptr, 0, -1}, {ExchangeItem::kMaxInt, mx, 2, -1}}, nullptr);
    if (rc != apex::kOk) return fail("issue: " + x.error());
    for (double v : all) if (v != total) return fail("sum to every rank: " + std::to_string(v));
    if (rank == 1) for (double v : rooted) if (v != total) return fail("sum to root 1: " + std::to_string(v));
    if (mx[0] != world || mx[1] != world) return fail("max: " + std::to_string(mx[0]) + ", " + std::to_string(mx[1]));
    snprintf(msg, (size_t)msg_len, "rank %d of %d ok: sum %g max %d", rank, world, all[0], mx[0]);
    return 0;
}
