// host_thread.hpp -- a context's own host thread: a run that needs the host after every iteration (the reference-order modes of ICP and of the dense tracker)
// proceeds there, so that an "enqueue" call returns at once and several contexts run side by side.
#pragma once
#include <exception>
#include <thread>
#include <utility>

#include "common.hpp"

namespace op {

struct HostThread {
    bool active = false; // a run has been started and not yet joined: the thread owns the context
    // Runs fn() (which returns an OP_* code) on a new thread.  Never throws: std::system_error (no thread to be had) must not cross the extern "C" boundary --
    // then fn is destroyed without having run and the answer is OP_ERR_INVALID, "<what>: <reason>".
    template <class F>
    int start(const char* what, F fn) {
        active = true; rc_ = OP_OK; err_[0] = 0;
        try {
            th_ = std::thread([this, fn = std::move(fn)]() mutable {
                rc_ = fn();
                if (rc_ != OP_OK) std::snprintf(err_, sizeof(err_), "%s", g_last_error); // (the error text is thread-local: hand it over)
            });
        } catch (const std::exception& e) {
            active = false;
            return fail(OP_ERR_INVALID, "%s: %s", what, e.what());
        }
        return OP_OK;
    }
    // waits for the run; its result, with its error text in the caller's g_last_error
    int join() {
        th_.join();
        active = false;
        return rc_ != OP_OK ? fail(rc_, "%s", err_) : OP_OK;
    }
private:
    std::thread th_;
    int rc_ = OP_OK;
    char err_[512] = "";
};

} // namespace op
