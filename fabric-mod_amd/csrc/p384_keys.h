// The registered P-384 keys of one context as the HOST keeps them (pure C++, no HIP; fabgpu_api.hip is the user,
// libfabgpu_hosttest.so shows it to tests/test_p384_keyed_host.py): a second instance of the unchanged KeySlots (key_slots.h) - ids
// are generation << 12 | slot, independent of the P-256 ids - the table and the name (qx || qy, 96 bytes) of every slot's tenant, and
// the SNAPSHOT a keyed launch carries: per slot below the high-water mark the live tenant's table and generation, or
// (nullptr, KTAB_GEN_NONE) for a slot between two tenants.  A snapshot is made from the book as it is at that moment and never
// edited: a retired key is gone from every snapshot made after the retirement, whatever the device still runs.
// With FABGPU_FLAG_P384_KEY_TABLES_16BIT a slot has a second address, the tenant's FINISHED 16-bit table (p384_tables16.h) or null; it
// travels in the same snapshot (snapshot16) and leaves with the tenant.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "key_slots.h"

namespace fab {

struct P384SlotSnap {       // 16 bytes, what p384_verify_keyed_kernel reads per slot (kernels.h P384KeyedLaunch)
    const uint32_t* tab;
    uint32_t gen;
    uint32_t pad;
};
constexpr uint32_t P384_GEN_NONE = 0xFFFFFFFFu;        // (== KTAB_GEN_NONE, kernels.h: no id carries it)
static_assert(P384_GEN_NONE > KeySlots::GEN_LAST, "no id may carry the generation word of a slot between two tenants");

class P384KeyBook {
public:
    explicit P384KeyBook(uint32_t gen_last = KeySlots::GEN_LAST) : slots(gen_last) {}
    KeySlots slots;

    bool lookup(const std::string& name, uint32_t* id) const {
        auto it = ids_.find(name);
        if (it == ids_.end()) return false;
        *id = it->second;
        return true;
    }
    // slots.next_slot() (>= 0, not DRAINING any more) gets `name` and its table; the new id
    uint32_t install(const std::string& name, uint32_t* tab) {
        const uint32_t slot = (uint32_t)slots.next_slot();
        if (slot >= tabs_.size()) {
            tabs_.resize((size_t)slot + 1, nullptr);
            tabs16_.resize((size_t)slot + 1, nullptr);
            names_.resize((size_t)slot + 1);
        }
        tabs_[slot] = tab;
        tabs16_[slot] = nullptr;
        names_[slot] = name;
        const uint32_t id = slots.take(slot);
        ids_[name] = id;
        return id;
    }
    // 0: retired, *tab (and *tab16, the tenant's 16-bit table or null) is what the slot's drain has to keep until no launch reads it;
    // 1: the id is not live
    int retire(uint32_t id, uint32_t** tab, uint32_t** tab16 = nullptr) {
        if (!slots.live(id)) return 1;
        const uint32_t slot = KeySlots::slot_of(id);
        ids_.erase(names_[slot]);
        names_[slot].clear();
        *tab = tabs_[slot];
        tabs_[slot] = nullptr;
        if (tab16) *tab16 = tabs16_[slot];
        n_tabs16_ -= tabs16_[slot] ? 1u : 0u;
        tabs16_[slot] = nullptr;
        slots.retire(id);
        return 0;
    }
    uint32_t* table(uint32_t id) const { return slots.live(id) ? tabs_[KeySlots::slot_of(id)] : nullptr; }
    // The optional 16-bit table of a live key: set once, by whoever has seen its build finish.  false: the id is not live (any more).
    bool set_table16(uint32_t id, uint32_t* tab16) {
        if (!slots.live(id) || !tab16 || tabs16_[KeySlots::slot_of(id)]) return false;
        tabs16_[KeySlots::slot_of(id)] = tab16;
        n_tabs16_++;
        return true;
    }
    uint32_t* table16(uint32_t id) const { return slots.live(id) ? tabs16_[KeySlots::slot_of(id)] : nullptr; }
    uint32_t n_tables16() const { return n_tabs16_; }
    // the second address per slot of a snapshot: the live tenant's finished 16-bit table, or null
    std::vector<const uint32_t*> snapshot16() const {
        std::vector<const uint32_t*> s(slots.high_water(), nullptr);
        for (uint32_t k = 0; k < s.size(); k++)
            if (slots.state(k) == KeySlots::LIVE) s[k] = tabs16_[k];
        return s;
    }
    std::vector<P384SlotSnap> snapshot() const {
        std::vector<P384SlotSnap> s(slots.high_water());
        for (uint32_t k = 0; k < s.size(); k++) {
            const bool live = slots.state(k) == KeySlots::LIVE;
            s[k] = P384SlotSnap{live ? tabs_[k] : nullptr, live ? slots.generation(k) : P384_GEN_NONE, 0};
        }
        return s;
    }

private:
    std::vector<uint32_t*> tabs_;
    std::vector<uint32_t*> tabs16_;
    uint32_t n_tabs16_ = 0;
    std::vector<std::string> names_;
    std::map<std::string, uint32_t> ids_;
};

}  // namespace fab
