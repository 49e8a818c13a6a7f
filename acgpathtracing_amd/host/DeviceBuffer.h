// DeviceBuffer.h — owner of one pt_device_malloc allocation in a render context: freed when it goes out of scope, on an
// exception's way out too.  `what` names the command the buffer serves ("sweep", "denoise", ...): a failing allocation or copy
// throws acgpt::Exception(what + ": " + pt_last_error(ctx)), and ptRequire() does the same for the library calls in between.
// A size of 0 allocates nothing: the pointer is null, and uploads and downloads of 0 bytes are no calls.
#pragma once
#include <cstddef>
#include <string>
#include "Exception.h"

namespace acgpt {

inline void ptRequire(pt_ctx* ctx, int rc, const std::string& what)
{
    if (rc != 0) throw Exception(what + ": " + pt_last_error(ctx));
}

class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(pt_ctx* ctx, size_t bytes, const std::string& what) : m_ctx(ctx), m_what(what)
    {
        if (bytes != 0) ptRequire(m_ctx, pt_device_malloc(m_ctx, &m_ptr, bytes), m_what);
    }
    ~DeviceBuffer() { reset(); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : m_ctx(o.m_ctx), m_ptr(o.m_ptr), m_what(std::move(o.m_what)) { o.m_ptr = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) { reset(); m_ctx = o.m_ctx; m_ptr = o.m_ptr; m_what = std::move(o.m_what); o.m_ptr = nullptr; }
        return *this;
    }

    void upload(const void* host, size_t bytes) { if (bytes != 0) ptRequire(m_ctx, pt_copy_to_device(m_ctx, m_ptr, host, bytes), m_what); }
    void download(void* host, size_t bytes) const { if (bytes != 0) ptRequire(m_ctx, pt_copy_to_host(m_ctx, host, m_ptr, bytes), m_what); }
    void reset() { if (m_ptr) pt_device_free(m_ctx, m_ptr); m_ptr = nullptr; }

    void* get() const { return m_ptr; }
    template <typename T> T* as() const { return static_cast<T*>(m_ptr); }
    explicit operator bool() const { return m_ptr != nullptr; }

private:
    pt_ctx* m_ctx = nullptr;
    void* m_ptr = nullptr;
    std::string m_what;
};

}  // namespace acgpt
