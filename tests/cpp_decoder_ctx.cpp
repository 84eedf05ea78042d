// The decoder classes of the C++ mirror (include/dark.hpp) make decoder contexts: Decoder::new (src/block/dc.rs:106-115, src/block/raw.rs)
// takes the inverse path's workspace only, the encoders and saca::Constructor take a full context as before.
// Built and run by tests/test_gpu_decoder_ctx.py on the GPU box.  argv[1] = path of the LICENSE fixture.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "dark.hpp"

using Bytes = std::vector<uint8_t>;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int sized_as_a_decoder(dark::detail::Ctx &ctx, size_t n) {
    dk_stats st;
    CHECK(ctx.purpose() == DK_CTX_DECODER);
    CHECK(dk_get_stats(ctx.get(), &st) == DK_OK);
    CHECK(st.ws_size_bytes == dk_workspace_bytes(DK_CTX_DECODER, n, 1));
    CHECK(st.ws_peak_bytes > 0 && st.ws_peak_bytes <= st.ws_size_bytes);
    CHECK(4 * st.ws_size_bytes <= dk_workspace_bytes(DK_CTX_FULL, n, 1));
    return 0;
}

template <class M>
static int roundtrip(M model, const Bytes &data, bool any_byte) {
    dark::block::dc::Encoder<M> enc(data.size(), model, 0, any_byte);
    auto [writer, err] = enc.encode(data, Bytes());
    err.unwrap();
    dark::block::dc::Decoder<M> dec(data.size(), enc.model, 0, any_byte);
    auto [reader, output, err2] = dec.decode(writer, Bytes());
    (void)reader;
    err2.unwrap();
    CHECK(output == data);
    return sized_as_a_decoder(dec.context(), data.size());
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    Bytes text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    CHECK(text.size() == 1083);
    if (roundtrip(dark::model::exp::Model(), text, false)) return 1;
    if (roundtrip(dark::model::ybs::Model(), text, false)) return 1;
    if (roundtrip(dark::model::dark::Model(), text, false)) return 1;
    if (roundtrip(dark::model::simple::Model(), text, false)) return 1;
    Bytes with_ff = text;
    with_ff[7] = with_ff[500] = with_ff.back() = 0xFF;
    if (roundtrip(dark::model::dark::Model(), with_ff, true)) return 1;
    {
        dark::block::raw::Encoder<dark::model::bbb::Model> enc(text.size(), dark::model::bbb::Model());
        auto [writer, err] = enc.encode(text, Bytes());
        err.unwrap();
        dark::block::raw::Decoder<dark::model::bbb::Model> dec(text.size(), enc.model);
        auto [reader, output, err2] = dec.decode(writer, Bytes());
        (void)reader;
        err2.unwrap();
        CHECK(output == text);
        if (sized_as_a_decoder(dec.context(), text.size())) return 1;
        // what a decoder's context refuses, and that it goes on afterwards
        try { dark::bwt::transform(dec.context(), text); return 1; } catch (const dark::Error &e) { CHECK(e.code == DK_E_ARG); }
        CHECK(dec.context().error().find("dk_bwt_forward") == 0 && dec.context().error().find("decoder context") != std::string::npos);
        auto [reader2, output2, err3] = dec.decode(writer, Bytes());
        (void)reader2;
        err3.unwrap();
        CHECK(output2 == text);
    }
    {   // the constructor's context is a full one, and serves the inverse as it always has
        dark::saca::Constructor con(text.size());
        CHECK(con.context().purpose() == DK_CTX_FULL);
        auto [L, origin] = dark::bwt::transform(con.context(), text);
        CHECK(dark::bwt::decode(con.context(), L, origin) == text);
    }
    std::puts("cpp decoder contexts ok");
    return 0;
}
