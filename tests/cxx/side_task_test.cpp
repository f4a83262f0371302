// csrc/side_task.h on its own: what the setup's overlap workers rely on.  Built twice by tests/test_side_task_host.py,
// under the thread sanitizer and under the address + undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "side_task.h"

using saamge_amd::SideTask;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

// how often join() throws a runtime_error with this text: 0 or 1
static int joins_throwing(SideTask &t, const std::string &what) {
    try {
        t.join();
    } catch (const std::runtime_error &e) {
        CHECK(what == e.what());
        return 1;
    }
    return 0;
}

static void exception_reaches_join_once(bool inline_now) {
    SideTask t;
    t.start([]() { throw std::runtime_error("from the worker"); }, inline_now);      // (must not leave start, inline or not)
    CHECK(t.pending());
    CHECK(joins_throwing(t, "from the worker") == 1);
    CHECK(!t.pending());
    CHECK(joins_throwing(t, "from the worker") == 0);      // a second join is quiet
    t.start([]() {}, inline_now);                          // ... and the slot is clean for the next task
    CHECK(joins_throwing(t, "from the worker") == 0);
}

static void destroyed_with_an_exception_pending() {
    for (int inline_now = 0; inline_now < 2; ++inline_now) {
        SideTask t;
        t.start([]() { throw std::runtime_error("nobody joins"); }, inline_now != 0);
    }      // neither throws nor terminates
    int done = 0;
    {
        SideTask t;
        t.start([&done]() { done = 1; });
    }      // the destructor waits for the work
    CHECK(done == 1);
}

static void inline_runs_on_the_calling_thread() {
    const std::thread::id me = std::this_thread::get_id();
    std::thread::id ran;
    SideTask t;
    t.start([&ran]() { ran = std::this_thread::get_id(); }, true);
    CHECK(ran == me);      // (already: inline work is done when start returns)
    t.join();
    t.start([&ran]() { ran = std::this_thread::get_id(); });
    t.join();
    CHECK(ran != me && ran != std::thread::id());
}

static void second_start_is_refused() {
    for (int inline_now = 0; inline_now < 2; ++inline_now) {
        SideTask t;
        int first = 0, second = 0;
        t.start([&first]() { first = 1; }, inline_now != 0);
        bool refused = false;
        try {
            t.start([&second]() { second = 1; });
        } catch (const std::logic_error &) { refused = true; }
        CHECK(refused);
        CHECK(t.pending());      // the first task is still there to be joined
        t.join();
        CHECK(first == 1 && second == 0);
    }
}

static void restart_and_visibility() {
    // plain (non-atomic) state written by the worker and read after join(): join() is the only synchronisation
    SideTask t;
    std::vector<int> v(64, 0);
    long sum = 0;
    for (int round = 1; round <= 100; ++round) {
        t.start([&v, &sum, round]() {
            for (int &x : v) x = round;
            sum += round;
        }, round % 10 == 0);
        CHECK(t.pending());
        t.join();
        CHECK(!t.pending());
        for (int x : v) CHECK(x == round);
    }
    CHECK(sum == 5050);
}

int main() {
    CHECK(!SideTask().pending());
    SideTask().join();      // nothing to wait for
    exception_reaches_join_once(false);
    exception_reaches_join_once(true);
    destroyed_with_an_exception_pending();
    inline_runs_on_the_calling_thread();
    second_start_is_refused();
    restart_and_visibility();
    std::printf("side task test ok\n");
    return 0;
}
