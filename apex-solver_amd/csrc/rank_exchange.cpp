// rank_exchange.cpp -- see rank_exchange.h
#include "rank_exchange.h"

namespace apex {

int RankExchange::issue(const ExchangeList& list, hipStream_t s) {
    if (!active()) return kOk;
    bool ok = comm_->group_start();
    for (const ExchangeItem& it : list) {
        if (!ok || it.n == 0) continue;
        if (it.op == ExchangeItem::kMaxInt) ok = comm_->all_reduce_max(static_cast<int*>(it.dev), it.n, s);
        else if (it.root >= 0) ok = comm_->reduce_sum(static_cast<double*>(it.dev), it.n, it.root, s);
        else ok = comm_->all_reduce_sum(static_cast<double*>(it.dev), it.n, s);
    }
    return done(ok && comm_->group_end());
}

}  // namespace apex
