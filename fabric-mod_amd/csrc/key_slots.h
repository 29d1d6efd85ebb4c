// Which slot of a context's key table a registered P-256 key gets, and under which id (pure C++, no HIP; fabgpu_api.hip is the user,
// libfabgpu_testhooks.so shows it to tests/test_key_slots.py).
//
// A key id is generation << 12 | slot.  A slot's first tenant has generation 0, so a context that never retires a key hands out
// 0, 1, 2 ... in registration order.  A retired slot is DRAINING until the owner has seen every launch that may still name its old id
// finish (drained()), then FREE; a registration takes the LOWEST slot that is DRAINING or FREE - whichever of the two it is - and only
// when there is none a slot that never had a tenant.  When the lowest one is still DRAINING the owner WAITS for it and does not pick
// another: the ids an allocator hands out then follow from the sequence of register / retire calls alone, never from how fast a device
// drained, and the devices of one provider, fed the same sequence, agree on every id.
// A slot whose tenant had the last generation is PARKED when that tenant retires: its ids are used up, it is never handed out again.
#pragma once
#include <cstdint>
#include <set>
#include <vector>

namespace fab {

class KeySlots {
public:
    static constexpr uint32_t SLOT_BITS = 12;
    static constexpr uint32_t MAX_SLOTS = 1u << SLOT_BITS;              // == FABGPU_MAX_KEYS: a cap on LIVE keys
    static constexpr uint32_t GEN_LAST = (1u << (32 - SLOT_BITS)) - 1;  // 20 bits of generation
    static constexpr uint32_t slot_of(uint32_t id) { return id & (MAX_SLOTS - 1); }
    static constexpr uint32_t gen_of(uint32_t id) { return id >> SLOT_BITS; }
    static constexpr uint32_t make_id(uint32_t gen, uint32_t slot) { return gen << SLOT_BITS | slot; }

    enum State : uint8_t { LIVE, DRAINING, FREE, PARKED };

    // gen_last: the last generation a slot may reach (tests shorten it; the product takes the default)
    explicit KeySlots(uint32_t gen_last = GEN_LAST) : gen_last_(gen_last > GEN_LAST ? GEN_LAST : gen_last) {}

    // the slot the next registration gets, or -1: MAX_SLOTS keys are live, or every slot that is not live is parked
    int64_t next_slot() const {
        if (!reclaimable_.empty()) return *reclaimable_.begin();
        return slots_.size() < MAX_SLOTS ? (int64_t)slots_.size() : -1;
    }
    // how many more registrations can succeed before a retirement
    uint32_t room() const { return (uint32_t)reclaimable_.size() + (MAX_SLOTS - (uint32_t)slots_.size()); }
    bool draining(uint32_t slot) const { return slot < slots_.size() && slots_[slot].state == DRAINING; }
    // the owner saw the slot's last launches finish
    void drained(uint32_t slot) {
        if (!draining(slot)) return;
        slots_[slot].state = FREE;
        n_draining_--;
    }
    // next_slot() becomes live (it must not be DRAINING any more); the new tenant's id
    uint32_t take(uint32_t slot) {
        if (slot == slots_.size()) {
            slots_.push_back(Slot{0, LIVE});
        } else {
            Slot& s = slots_[slot];
            reclaimable_.erase(slot);
            s.gen++;
            s.state = LIVE;
            n_reused_++;
        }
        n_live_++;
        return make_id(slots_[slot].gen, slot);
    }
    // 0: the id was live and is retired now (its slot is DRAINING, or PARKED after the last generation); 1: the id is not live
    int retire(uint32_t id) {
        const uint32_t slot = slot_of(id);
        if (slot >= slots_.size() || slots_[slot].state != LIVE || slots_[slot].gen != gen_of(id)) return 1;
        Slot& s = slots_[slot];
        n_live_--;
        if (s.gen >= gen_last_) {
            s.state = PARKED;
            n_parked_++;
        } else {
            s.state = DRAINING;
            n_draining_++;
            reclaimable_.insert(slot);
        }
        return 0;
    }
    bool live(uint32_t id) const {
        const uint32_t slot = slot_of(id);
        return slot < slots_.size() && slots_[slot].state == LIVE && slots_[slot].gen == gen_of(id);
    }
    State state(uint32_t slot) const { return slots_[slot].state; }
    uint32_t generation(uint32_t slot) const { return slots_[slot].gen; }
    uint32_t high_water() const { return (uint32_t)slots_.size(); }      // slots that ever had a tenant: what the kernels bound a slot by
    uint32_t n_live() const { return n_live_; }
    uint32_t n_draining() const { return n_draining_; }
    uint32_t n_parked() const { return n_parked_; }
    uint64_t n_reused() const { return n_reused_; }

private:
    struct Slot {
        uint32_t gen;
        State state;
    };
    uint32_t gen_last_;
    std::vector<Slot> slots_;
    std::set<uint32_t> reclaimable_;      // DRAINING or FREE
    uint32_t n_live_ = 0, n_draining_ = 0, n_parked_ = 0;
    uint64_t n_reused_ = 0;
};

}  // namespace fab
