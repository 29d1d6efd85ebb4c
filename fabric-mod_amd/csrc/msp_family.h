// The hash family of an MSP, as the block pass knows it (DESIGN.md 4.4 "Hash family"): a plain table mspid -> family under a lock of its
// own, set by fabgpu_csp_msp_hash_family and read by GPUCSP::P384PassStage once per identity a pass meets.  An MSP signs over the digest
// its SignatureHashFamily selects (msp/identities.go:216-224 getHashOpt): "SHA2" -> SHA-256, "SHA3" -> SHA3-256.  Every MSP is SHA2 until
// it is set otherwise; setting it back to SHA2 forgets it.
//
// Pure host code over strings: no provider state, no device.  csrc/hosttest_msp_family.cpp drives it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_set>

namespace fab {

// identity.getHashOpt's question.  "SHA2" / "SHA3" -> *sha3; anything else (nullptr reads as ""): false, and *err holds the reference's
// text.  "SHA3" while the provider does not serve the family (sha3_served false): false, and *err says who serves it.
inline bool ParseHashFamily(const char* family, bool sha3_served, bool* sha3, std::string* err) {
    const std::string f = family ? family : "";
    *sha3 = false;
    if (f == "SHA2") return true;
    if (f == "SHA3") {
        if (!sha3_served) {
            if (err) *err = "failed computing digest: SHA3 is served by bccsp/sw, not by the GPU provider";
            return false;
        }
        *sha3 = true;
        return true;
    }
    if (err) *err = "hash familiy not recognized [" + f + "]";               // (the reference's spelling)
    return false;
}

class MspFamilyTable {
   public:
    static constexpr size_t kMaxMspId = 1024;                // longest mspid the table takes (a longer one is SHA2, and cannot be set)
    // false: an mspid the table does not take (empty, or longer than kMaxMspId)
    bool Set(const std::string& mspid, bool sha3) {
        if (mspid.empty() || mspid.size() > kMaxMspId) return false;
        std::unique_lock<std::shared_mutex> lk(mu_);
        if (sha3) sha3_.insert(mspid);
        else sha3_.erase(mspid);
        n_.store(sha3_.size(), std::memory_order_release);
        return true;
    }
    // is this MSP of the SHA3 family?  (the bytes as a SerializedIdentity carries them: no terminator)
    bool Sha3(const uint8_t* mspid, size_t len) const {
        if (!mspid || len == 0 || len > kMaxMspId || !AnySha3()) return false;
        const std::string k((const char*)mspid, len);
        std::shared_lock<std::shared_mutex> lk(mu_);
        return sha3_.find(k) != sha3_.end();
    }
    bool Sha3(const std::string& mspid) const { return Sha3((const uint8_t*)mspid.data(), mspid.size()); }
    // no MSP is set SHA3: a pass need not read a single mspid (one relaxed-cost load, no lock)
    bool AnySha3() const { return n_.load(std::memory_order_acquire) != 0; }
    size_t CountSha3() const { return n_.load(std::memory_order_acquire); }

   private:
    mutable std::shared_mutex mu_;
    std::unordered_set<std::string> sha3_;                   // the MSPs that are not of the default family
    std::atomic<size_t> n_{0};                               // sha3_.size(), readable without the lock
};

}  // namespace fab
