// moved: the transcript of zkhost/transcript.hpp uses it too
#pragma once
#include "zkhost/sha256.hpp"
