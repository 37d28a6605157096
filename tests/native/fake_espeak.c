/* A stand-in for eSpeak NG's three entry points the text front-end loads at run time (frame_producer.cpp, Espeak): the "phonemes" of a
 * clause are the clause itself, so a test can feed speechPlayer_batch_setText IPA and know what the producer was given
 * (tests/test_alignment_host.py builds it as a shared library and names it in SPEECHPLAYER_ESPEAK_LIB).  Host only. */
#include <string.h>
int espeak_Initialize(int output, int buflength, const char* path, int options) { (void)output; (void)buflength; (void)path; (void)options; return 22050; }
int espeak_SetVoiceByName(const char* name) { (void)name; return 0; }
const char* espeak_TextToPhonemes(const void** textptr, int textmode, int phonememode)
{
    static char buf[4096];
    (void)textmode; (void)phonememode;
    strncpy(buf, (const char*)*textptr, sizeof buf - 1);
    buf[sizeof buf - 1] = 0;
    *textptr = 0;
    return buf;
}
