// host_threads.h -- the host threads of the JPEG entries (jpeg.hip, jpeg_enc.hip).
#pragma once
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

// items 0 .. n - 1 handed out in order to at most min(16, hardware threads) host threads, the caller's among them
template <class F>
void run_on_host_threads(size_t n, F f) {
    std::atomic<size_t> next{0};
    auto worker = [&]() { for (size_t t = next++; t < n; t = next++) f(t); };
    const size_t hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (size_t t = 1; t < std::min(hw, n); t++) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
}
