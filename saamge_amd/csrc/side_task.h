// One piece of work beside the calling thread (plain C++, no HIP): start it, go on, join it where its result is needed.
// Whatever the work throws is kept in the task and rethrown by join() on the joining thread.
#pragma once
#include <exception>
#include <stdexcept>
#include <thread>
#include <utility>

namespace saamge_amd {

class SideTask {
    std::thread t_;
    std::exception_ptr err_;
    bool pending_ = false;

  public:
    SideTask() = default;
    SideTask(const SideTask &) = delete;
    SideTask &operator=(const SideTask &) = delete;
    // joins what still runs and drops an exception nobody joined for.  Declare a task AFTER what its work refers to.
    ~SideTask() { if (t_.joinable()) t_.join(); }
    // fn on a thread of its own, or (inline_now) on the calling thread before start returns.  One task at a time.
    template <class F>
    void start(F fn, bool inline_now = false) {
        if (pending_) throw std::logic_error("SideTask: started again before it was joined");
        auto run = [this, fn = std::move(fn)]() mutable { try { fn(); } catch (...) { err_ = std::current_exception(); } };
        if (inline_now) run();
        else t_ = std::thread(std::move(run));
        pending_ = true;
    }
    // waits for the work and rethrows what it threw, once; nothing pending: nothing
    void join() {
        if (t_.joinable()) t_.join();
        pending_ = false;
        if (err_) std::rethrow_exception(std::exchange(err_, nullptr));
    }
    bool pending() const { return pending_; }
    static unsigned hardware_threads() { return std::thread::hardware_concurrency(); }
};

}  // namespace saamge_amd
