// gate_baton.h — the host half of the group gate chain (include/slideo_amd.h "Group gate order"): what one member's thread hands to
// the next.  A baton is published once (the predecessor's gate state lies in the group's pinned record) or failed once (the
// predecessor threw before it got that far); its one reader blocks in await until either.  Plain C++, no HIP include
// (tools/group_gate_chain_hostcheck.cpp runs it with real threads).
#pragma once
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <stdexcept>
#include <string>

namespace slideo {

class GateBaton {
public:
    // the state is handed over: releases await.  Later calls of publish or fail change nothing.
    void publish() { settle(PUBLISHED, std::string()); }
    // the predecessor failed: await throws std::runtime_error(why)
    void fail(const std::string& why) { settle(FAILED, why); }
    // blocks until publish or fail; returns the seconds it blocked
    double await() {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return state_ != PENDING; });
        if (state_ == FAILED) throw std::runtime_error(why_);
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    bool settled() {
        std::lock_guard<std::mutex> lk(mu_);
        return state_ != PENDING;
    }
    void reset() {
        std::lock_guard<std::mutex> lk(mu_);
        state_ = PENDING;
        why_.clear();
    }

private:
    enum State { PENDING, PUBLISHED, FAILED };
    void settle(State s, const std::string& why) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (state_ != PENDING) return;
            state_ = s;
            why_ = why;
        }
        cv_.notify_all();
    }
    std::mutex mu_;
    std::condition_variable cv_;
    State state_ = PENDING;
    std::string why_;
};

// A member's hold on the baton it owes its successor: dropped unpublished — the member threw, or returned without a last unit — it
// fails the baton, so the successor's thread ends too.
class GateBatonGuard {
public:
    explicit GateBatonGuard(GateBaton* b, std::string why = "the predecessor in the group gate chain failed before it handed its gate state over")
        : b_(b), why_(std::move(why)) {}
    GateBatonGuard(const GateBatonGuard&) = delete;
    GateBatonGuard& operator=(const GateBatonGuard&) = delete;
    ~GateBatonGuard() { if (b_) b_->fail(why_); }      // (a published baton ignores it)
    void publish() { if (b_) b_->publish(); }

private:
    GateBaton* b_;
    std::string why_;
};

}  // namespace slideo
